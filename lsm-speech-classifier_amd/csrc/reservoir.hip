// Host side of the reservoir C ABI (include/lsm_hip.h): handle creation (CSC upload, per-layout tables), layout choice and
// kernel launch.  The kernels live in lif_kernel.h (sparse CSC scatter), lif_dense.h (dense rows), lif_ring.h (ring rows in
// quads) and lif_pair.h (ring rows in pair blocks), what they share in lif_common.h; the lif_variant_*, lif_dense_*,
// lif_ring_*, lif_pair_* and lif_pair_wide_*.hip translation units instantiate them.
#include "lif_kernel.h"
#include "lif_dense.h"
#include "lif_ring.h"
#include "lif_pair.h"
#include "reservoir_facts.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

using lsm_lif::LifArgs;
using lsm_lif::lif_fn_t;
using lsm_lif::IN_REG_SLOTS;

namespace {

// The numbers of the ABI: lsm_reservoir_set_kernel's mode, and the kernel lsm_reservoir_plan / _kernel_in_use report.
enum KernelMode { MODE_AUTO = 0, MODE_SPARSE = 1, MODE_DENSE = 2, MODE_RING = 3, MODE_RING_CONTIGUOUS = 4, MODE_RING_PAIRS = 5,
                  MODE_RING_QUADS = 6 };
enum PlannedKernel { KERNEL_NONE = 0, KERNEL_SPARSE = 1, KERNEL_DENSE = 2, KERNEL_RING = 3 };

lif_fn_t pick_kernel(int sl, int wpc, bool inreg, bool seglds, bool state)
{
    if (inreg) return seglds ? lsm_lif::pick_lif_11(sl, wpc, state) : lsm_lif::pick_lif_10(sl, wpc, state);
    return seglds ? lsm_lif::pick_lif_01(sl, wpc, state) : lsm_lif::pick_lif_00(sl, wpc, state);
}

// Owning device pointer: move-only, hipFree when it goes.  Every table of a handle is one.
struct DevFree {
    void operator()(void *p) const { (void)hipFree(p); }
};
template <typename T>
using DevPtr = std::unique_ptr<T, DevFree>;

struct Variant {            // per waves-per-clip layout
    int wpc = 0, sl = 0, einw = 0;
    DevPtr<uint32_t> seg;
    DevPtr<uint16_t> segoff;
    DevPtr<float> leak;
    DevPtr<int> oslot;
    DevPtr<uint32_t> in_ent;
    DevPtr<uint32_t> inmask;         // (npad, 4) input-channel masks, only when C <= 128 and sl <= 4
    bool incol = false;              // the masks use the coloured bit positions of lsm_reservoir::inperm (INMODE 3)
};

struct RingVariant {        // per waves-per-clip layout of the ring-row kernel (lif_ring.h)
    int wpc = 0, ql = 0, einw = 0;
    bool strided = false;            // quad ownership: wave w owns quads w, w+wpc, ... (else w*ql .. w*ql+ql-1)
    size_t n_rem = 0;                // list entries (synapses outside the ring window)
    DevPtr<uint32_t> rem_ptr;        // (N*wpc + 1) first list entry of (row, wave)
    DevPtr<uint2> rem;               // synapses outside the ring window: {LDS byte offset of the accumulator, weight bits}
    DevPtr<float> leak;
    DevPtr<int> oslot;
    DevPtr<uint32_t> in_ent;         // (wpc, einw) packed input-map entries (lsm_lif::ring_pack_entry)
    DevPtr<uint32_t> inmask;         // (npad, 4) input-channel masks in neuron order: the INMASK kernel form (C <= 128, uniform
                                     // leak, strided ownership, <= 2 quads per wave), else null
    bool incol = false;              // the masks use the coloured bit positions of lsm_reservoir::inperm
};

struct PairVariant {        // per waves-per-clip layout of the pair-block ring kernel (lif_pair.h)
    int wpc = 0, bl = 0;             // wave w owns the 128-neuron blocks w, w+wpc, ...: bl of them
    size_t n_rem = 0;                // list entries (synapses outside the ring window)
    DevPtr<uint4> rec;               // (N*wpc) row records (lsm_lif::pair_record)
    DevPtr<uint2> rem;               // {LDS byte offset of the accumulator, weight bits}, (row, wave) major
    DevPtr<int> oslot;
    DevPtr<float> leak;              // (npad) leak coefficients when they differ between neurons, else null
    DevPtr<uint32_t> inmask;         // (npad, 4) input-channel masks in neuron order, or {posmask, P0, P1, P2} (inform 3)
    int inform = 0;                  // the kernel's INMASK: 1 masks at natural positions, 2 at the coloured positions of
                                     // lsm_reservoir::inperm, 3 bit planes over coloured positions (129..256 channels)
};

}  // namespace

// Dense presynaptic rows from the device copy of the CSC arrays: block j scatters column j into row j.
__global__ __launch_bounds__(256) void build_dense_rows_kernel(const uint32_t *__restrict__ rowptr,
                                                               const uint2 *__restrict__ syn, int ld,
                                                               float *__restrict__ wt)
{
    const uint32_t j = blockIdx.x;
    for (uint32_t e = rowptr[j] + threadIdx.x; e < rowptr[j + 1]; e += blockDim.x) {
        const uint2 s = syn[e];
        wt[(size_t)j * ld + s.x] = __uint_as_float(s.y);
    }
}

struct lsm_reservoir {
    int N = 0, C = 0, n_out = 0, refractory = 0, burst_isi_max = 0;
    float theta = 0, w_in = 0;
    int device = 0;
    int cus = 0;            // compute units of that device
    size_t nnz = 0;
    DevPtr<uint2> syn;
    DevPtr<uint32_t> rowptr;
    DevPtr<float> wt;       // dense rows by presynaptic neuron (N, ld), small reservoirs only
    int ld = 0;
    // ring rows (lif_ring.h): per presynaptic neuron the dense ring window from the 256-aligned start of
    // j-H up to j+H, plus per-layout lists of the synapses outside it
    DevPtr<float> band;
    uint32_t band_pitch = 0;
    double band_bytes_sum = 0;       // sum over rows of the window bytes that exist (what a spike's window loads can touch)
    int band_h = 0, band_nq = 0, band_wsq = 0;
    // INMODE 3 of the dense kernel: bit position of every input channel in the step's input bit row such that the
    // channels feeding one neuron sit at different positions mod 32 (colour_input_channels); null when no such
    // assignment was found (then the masks keep the natural positions, INMODE 2)
    DevPtr<uint8_t> inperm;
    bool leak_uniform = false;       // every neuron has the same leak coefficient (leak_u): the reference's default
    float leak_u = 0.0f;
    KernelMode mode = MODE_AUTO;     // MODE_RING_CONTIGUOUS: ring rows with contiguous quad ownership only (tests);
                                     // MODE_RING_PAIRS: pair blocks only (lif_pair.h); MODE_RING_QUADS: quads only (lif_ring.h,
                                     // either ownership)
    Variant var[5];         // wpc = 1, 2, 4, 8, 16 (wpc == 0: not available)
    RingVariant rvar[8];    // wpc = 2, 4, 8, 16, contiguous [0..3] and strided [4..7] quad ownership
    PairVariant pvar[3];    // wpc = 4, 8, 16: pair blocks (lif_pair.h), C <= 256 (above 128 only with a colouring)
};

static size_t ring_lds_bytes(const lsm_reservoir *h, const RingVariant &v, int T);

// reservoir_facts.h: for readout.hip, whose window launch folds this reservoir's records
ReservoirRecordFacts reservoir_record_facts(const lsm_reservoir *h) { return {h->n_out, h->burst_isi_max, h->device}; }

static bool has_ring(const lsm_reservoir *h)
{
    for (const auto &v : h->rvar)
        if (v.wpc) return true;
    return false;
}
static bool has_pairs(const lsm_reservoir *h)
{
    for (const auto &v : h->pvar)
        if (v.wpc) return true;
    return false;
}

// ring rows: on request, or by default when the dense table no longer fits the XCDs' L2 caches together
// (32 MB) -- from there on the dense rows are bound by the bytes of the row gathers, of which the ring
// format moves a quarter (N = 4000: window 3.6 KB + list 0.6 KB against 16 KB per row)
constexpr size_t RING_AUTO_MIN_DENSE_BYTES = (size_t)32 << 20;

template <typename T>
static int upload(DevPtr<T> *dst, const std::vector<T> &src)
{
    T *p = nullptr;
    LSM_CHECK_HIP(hipMalloc(reinterpret_cast<void **>(&p), std::max<size_t>(1, src.size()) * sizeof(T)));
    dst->reset(p);
    if (!src.empty())
        LSM_CHECK_HIP(hipMemcpy(p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return LSM_OK;
}

// Allocate and fill the dense row table of a handle that does not have it yet (synchronous: handle set-up, not a
// launch function).
static int ensure_dense_rows(lsm_reservoir *h)
{
    if (h->wt || h->ld <= 0) return LSM_OK;
    int dev_now = -1;
    LSM_CHECK_HIP(hipGetDevice(&dev_now));
    LSM_REQUIRE(dev_now == h->device, "reservoir handle lives on device %d but the current device is %d",
                h->device, dev_now);
    const size_t bytes = (size_t)h->N * (size_t)h->ld * sizeof(float);
    float *p = nullptr;
    LSM_CHECK_HIP(hipMalloc(reinterpret_cast<void **>(&p), bytes));
    DevPtr<float> wt(p);
    hipError_t e = hipMemset(p, 0, bytes);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(build_dense_rows_kernel, dim3(h->N), dim3(256), 0, nullptr, h->rowptr.get(), h->syn.get(), h->ld, p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        lsm_set_error("building the dense row table failed: %s", hipGetErrorString(e));
        return LSM_ERR_HIP;
    }
    h->wt = std::move(wt);
    return LSM_OK;
}

// Bit positions for the input channels of the dense kernel's INMODE 3 (C <= 128) and of the pair-block kernel's bit
// planes (C <= 256, lif_pair.h INMASK 3): position p = word * 32 + bit with
// word < ceil(C / 32), such that the channels feeding ONE neuron all have different `bit`s.  Then the words
// (mask_w & row_w) of a neuron have no set bit in common and popcount(m0&r0) + ... + popcount(m3&r3) =
// popcount((m0&r0) | (m1&r1) | (m2&r2) | (m3&r3)): one v_and, three v_and_or and one v_bcnt per neuron and step
// instead of four v_and, four v_bcnt and an add.  This is an equitable colouring of the channels' conflict graph
// (two channels conflict when they share a target) with 32 colours of ceil(C/32) places each; greedy by conflict
// degree with a one-move repair finds one for every input map tried (N = 256..4000, C = 32..128; N = 1024..8000,
// C = 129..256, where C = 256 forces exactly 8 channels per colour).  Returns false when it does not: the caller keeps
// the natural positions (INMODE 2; above 128 channels there is then no pair-block layout).
static bool colour_input_channels(int N, int C, const int32_t *in_tgt, int in_fanout, std::vector<uint8_t> *perm)
{
    if (C > 256) return false;
    const int cap = (C + 31) / 32;
    std::vector<std::vector<int>> chans_of(N);
    for (int c = 0; c < C; ++c)
        for (int d = 0; d < in_fanout; ++d) chans_of[in_tgt[(size_t)c * in_fanout + d]].push_back(c);
    std::vector<std::vector<char>> adj(C, std::vector<char>(C, 0));
    std::vector<int> deg(C, 0);
    for (const auto &l : chans_of)
        for (int x : l)
            for (int y : l)
                if (x != y && !adj[x][y]) { adj[x][y] = 1; ++deg[x]; }
    std::vector<int> order(C);
    for (int c = 0; c < C; ++c) order[c] = c;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return deg[x] > deg[y]; });
    std::vector<int> col(C, -1), cnt(32, 0);
    auto used_by_neighbours = [&](int c, int skip) {
        uint32_t used = 0u;
        for (int y = 0; y < C; ++y)
            if (adj[c][y] && col[y] >= 0 && y != skip) used |= 1u << col[y];
        return used;
    };
    for (int c : order) {
        const uint32_t used = used_by_neighbours(c, -1);
        int best = -1;
        for (int k = 0; k < 32; ++k)
            if (!((used >> k) & 1u) && cnt[k] < cap && (best < 0 || cnt[k] < cnt[best])) best = k;
        if (best < 0) {
            // every colour free of c's neighbours is full: move one member of such a colour elsewhere
            for (int k = 0; k < 32 && best < 0; ++k) {
                if ((used >> k) & 1u) continue;
                for (int v = 0; v < C && best < 0; ++v) {
                    if (col[v] != k) continue;
                    const uint32_t uv = used_by_neighbours(v, -1);
                    for (int q = 0; q < 32; ++q)
                        if (q != k && !((uv >> q) & 1u) && cnt[q] < cap && !adj[v][c]) {
                            col[v] = q; ++cnt[q]; --cnt[k];
                            best = k;
                            break;
                        }
                }
            }
            if (best < 0) return false;
        }
        col[c] = best;
        ++cnt[best];
    }
    // place the members of a colour in different words; verify before trusting the result
    perm->assign(C, 0);
    std::vector<int> next(32, 0);
    for (int c = 0; c < C; ++c) (*perm)[c] = (uint8_t)(next[col[c]]++ * 32 + col[c]);
    for (const auto &l : chans_of) {
        uint32_t seen = 0u;
        for (int x : l) {
            const uint32_t bit = 1u << ((*perm)[x] & 31);
            if (seen & bit) return false;
            seen |= bit;
        }
    }
    std::vector<char> taken(cap * 32, 0);
    for (int c = 0; c < C; ++c) {
        if ((*perm)[c] >= cap * 32 || taken[(*perm)[c]]) return false;
        taken[(*perm)[c]] = 1;
    }
    return true;
}

// What lsm_reservoir_create is given to build tables from (lsm_debug_pair_layout and lsm_debug_pair_inputs fill in the part
// their tables need).
struct Network {
    int N = 0, C = 0;
    const int32_t *csc_ptr = nullptr, *csc_post = nullptr;
    const float *csc_w = nullptr, *leak = nullptr;
    const int32_t *in_tgt = nullptr;
    int in_fanout = 0;
    const int32_t *out_idx = nullptr;
    int n_out = 0;
    size_t nnz = 0;
    const uint8_t *perm = nullptr;      // (C) coloured bit position of every channel (colour_input_channels), null: natural
};

static uint32_t weight_bits(float w)
{
    uint32_t bits;
    std::memcpy(&bits, &w, 4);
    return bits;
}

// (npad) leak coefficients / output slots in neuron order; padding neurons leak 0 and have no slot (-1)
static std::vector<float> padded_leak(const Network &net, int npad)
{
    std::vector<float> lk(npad, 0.0f);
    std::copy(net.leak, net.leak + net.N, lk.begin());
    return lk;
}
static std::vector<int> output_slots(const Network &net, int npad)
{
    std::vector<int> os(npad, -1);
    for (int o = 0; o < net.n_out; ++o) os[net.out_idx[o]] = o;
    return os;
}

// Per-neuron channel masks (npad, 4) in neuron order, C <= 128: bit p of neuron i's four words = the channel at position p
// (net.perm, else its own number) feeds neuron i -- INMODE 2 / 3 of the dense kernel, INMASK 1 / 2 of the ring and pair
// kernels.  Returns `distinct`: no channel names a neuron twice (SPEC.md 2.4 draws targets without replacement); the words
// hold one bit per (channel, neuron) pair, so a map that does has no mask form and `im` is not to be used.
static bool channel_masks(const Network &net, int npad, std::vector<uint32_t> *im)
{
    im->assign((size_t)npad * 4, 0u);
    for (int c = 0; c < net.C; ++c)
        for (int d = 0; d < net.in_fanout; ++d) {
            const int tgt = net.in_tgt[(size_t)c * net.in_fanout + d];
            const int pc = net.perm ? net.perm[c] : c;          // bit position of channel c in the input bit row
            uint32_t &word = (*im)[(size_t)tgt * 4 + (pc >> 5)];
            if (word & (1u << (pc & 31))) return false;
            word |= 1u << (pc & 31);
        }
    return true;
}

// The channel masks of a layout, uploaded when the map has them (channel_masks); *incol: at the coloured positions.
static int upload_channel_masks(const Network &net, int npad, DevPtr<uint32_t> *inmask, bool *incol)
{
    std::vector<uint32_t> im;
    if (!channel_masks(net, npad, &im)) return LSM_OK;
    *incol = net.perm != nullptr;
    return upload(inmask, im);
}

// The input map shared out by owner wave: (wpc, einw) words, entry(c, i) for every (channel c -> neuron i) pair of wave
// wave_of(i) in channel order, every wave's part padded with pad(index) to einw, a multiple of `block`.  Returns einw.
template <typename WaveOf, typename Entry, typename Pad>
static int wave_entries(const Network &net, int wpc, int block, WaveOf wave_of, Entry entry, Pad pad, std::vector<uint32_t> *ent)
{
    std::vector<std::vector<uint32_t>> per(wpc);
    for (int c = 0; c < net.C; ++c)
        for (int d = 0; d < net.in_fanout; ++d) {
            const int tgt = net.in_tgt[(size_t)c * net.in_fanout + d];
            per[wave_of(tgt)].push_back(entry(c, tgt));
        }
    size_t mx = 1;
    for (auto &pp : per) mx = std::max(mx, pp.size());
    const int einw = (int)((mx + block - 1) / block * block);
    ent->resize((size_t)wpc * einw);
    for (size_t e = 0; e < ent->size(); ++e) (*ent)[e] = pad(e);
    for (int w = 0; w < wpc; ++w)
        std::copy(per[w].begin(), per[w].end(), ent->begin() + (size_t)w * einw);
    return einw;
}

// ---- ring-row geometry and the pair-block tables: host arithmetic only (no HIP call), shared by lsm_reservoir_create and
// lsm_debug_pair_layout, which lets a CPU test apply every row from the tables alone (tests/test_pair_layout.py) ----
struct RingGeometry {
    int H = 0, NQ = 0, NP = 0, wsq = 0;
    uint32_t pitch = 0;
    std::vector<int> a4v, nbytes;       // per row: 32-aligned first target of the window; bytes of the row that exist
    // byte offset of synapse (j -> i) in row j, or -1 when i lies outside the stored window
    long win_off(int j, int i) const
    {
        int p = i - a4v[j]; p += p < 0 ? NP : 0;
        const long off = (long)p * 4;
        return off < nbytes[j] ? off : -1;
    }
};

// Window half-width H = half the mean out-degree (k/2 of a small-world graph).  Row j covers the targets from the
// 32-aligned start of (j-H) mod N up to (j+H) mod N along the ring padded to NQ quads of 256.  False when the reservoir is
// not ring-like enough for the format (the plain window must hold most of the synapses and be a real saving).
static bool ring_geometry(const Network &net, RingGeometry *g)
{
    const int N = net.N;
    const size_t nnz = net.nnz;
    const int H = (int)((nnz / (size_t)N + 1) / 2);
    const int wd = 2 * H + 1;
    const int NQ = (N + 255) / 256;
    size_t inside = 0;
    for (int j = 0; j < N; ++j)
        for (int e = net.csc_ptr[j]; e < net.csc_ptr[j + 1]; ++e) {
            int q = net.csc_post[e] - (j - H);
            q = q < 0 ? q + N : (q >= N ? q - N : q);
            inside += q < wd;
        }
    if (!(H >= 1 && 2 * wd <= N && NQ >= 2 && nnz > 0 && inside * 10 >= nnz * 6)) return false;
    // geometry per row: a4 (32-aligned first target of the window: 128 bytes), bytes that exist (up to the window's
    // end along the padded ring of NQ*256 positions, 16-byte granules), quads the window touches
    g->H = H; g->NQ = NQ; g->NP = NQ * 256;
    g->a4v.assign(N, 0); g->nbytes.assign(N, 0);
    int wsq = 0, maxb = 0;
    for (int j = 0; j < N; ++j) {
        int a0 = j - H; a0 += a0 < 0 ? N : 0;
        int b0 = j + H; b0 -= b0 >= N ? N : 0;
        const int a4 = a0 & ~31;
        int span = b0 - a4; span += span < 0 ? g->NP : 0;
        g->a4v[j] = a4;
        g->nbytes[j] = ((span >> 2) + 1) * 16;
        maxb = std::max(maxb, g->nbytes[j]);
        wsq = std::max(wsq, (((a4 & 255) + span) >> 8) + 1);
    }
    g->wsq = wsq;
    g->pitch = ((uint32_t)maxb + 127u) & ~127u;         // every row starts on a 128-byte line
    return wsq < NQ;
}

static void ring_windows(const Network &net, const RingGeometry &g, std::vector<float> *band)
{
    band->assign((size_t)net.N * (g.pitch / 4), 0.0f);
    for (int j = 0; j < net.N; ++j)
        for (int e = net.csc_ptr[j]; e < net.csc_ptr[j + 1]; ++e) {
            const long off = g.win_off(j, net.csc_post[e]);
            if (off >= 0) (*band)[(size_t)j * (g.pitch / 4) + (size_t)(off / 4)] = net.csc_w[e];
        }
}

// The synapses outside the ring windows as lists per (row j, wave w), unpadded: rptr[j*wpc + w] = first entry of the list,
// entries {acc_byte(target), weight bits} in ascending target order.  wave_of(i): the wave that owns neuron i in the layout;
// acc_byte(i): LDS byte offset of its accumulator.  Returns the longest list (the kernels give a list entry a lane: the
// callers refuse more than 64).
template <typename WaveOf, typename AccByte>
static int outside_lists(const Network &net, int wpc, const RingGeometry &g, WaveOf wave_of, AccByte acc_byte,
                         std::vector<uint32_t> *rptr, std::vector<uint2> *rem)
{
    rptr->assign((size_t)net.N * wpc + 1, 0u);
    int emax = 0;
    for (int j = 0; j < net.N; ++j)
        for (int e = net.csc_ptr[j]; e < net.csc_ptr[j + 1]; ++e)
            if (g.win_off(j, net.csc_post[e]) < 0)
                emax = std::max(emax, (int)++(*rptr)[(size_t)j * wpc + wave_of(net.csc_post[e]) + 1]);
    for (size_t q = 1; q < rptr->size(); ++q) (*rptr)[q] += (*rptr)[q - 1];
    rem->assign(std::max<size_t>(1, rptr->back()), make_uint2(0u, 0u));
    std::vector<uint32_t> fill(rptr->begin(), rptr->end() - 1);
    for (int j = 0; j < net.N; ++j)
        for (int e = net.csc_ptr[j]; e < net.csc_ptr[j + 1]; ++e) {
            const int i = net.csc_post[e];
            if (g.win_off(j, i) < 0)
                (*rem)[fill[(size_t)j * wpc + wave_of(i)]++] = make_uint2(acc_byte(i), weight_bits(net.csc_w[e]));
        }
    return emax;
}

// Blocks per wave of a pair-block layout with `wpc` waves: the 2*NQ blocks of 128 neurons shared out evenly (the residues
// must survive the ring's wrap), a wave at most four blocks (8 neurons per lane).  0 = no such layout.
static int pair_blocks_per_wave(int NQ, int wpc)
{
    const int NB = 2 * NQ;
    return (NB % wpc == 0 && NB / wpc <= 4) ? NB / wpc : 0;
}

// Pair blocks (lif_pair.h): the windows shared out in 128-neuron blocks, wave w owning the blocks w, w+wpc, ...
// (pair_blocks_per_wave), a window must not touch more than wpc blocks, a (row, wave) list at most 64 entries.  Returns the
// blocks per wave, 0 = no layout.
static int pair_lists(const Network &net, int wpc, const RingGeometry &g, std::vector<uint32_t> *rptr, std::vector<uint2> *rem)
{
    int wsb = 0;
    for (int j = 0; j < net.N; ++j) wsb = std::max(wsb, (((g.a4v[j] & 127) + (g.nbytes[j] / 4 - 1)) >> 7) + 1);
    const int bl = pair_blocks_per_wave(g.NQ, wpc);
    if (!bl || wsb > wpc) return 0;
    const int emax = outside_lists(net, wpc, g, [&](int i) { return lsm_lif::pair_wave_of_block(i >> 7, wpc); },
                                   [](int i) { return lsm_lif::pair_acc_byte(i); }, rptr, rem);
    if (emax > 64) return 0;                                 // one lane per list entry
    if ((uint64_t)rptr->back() * 8u >= (1ull << 32)) return 0;     // a record holds the low 32 bits of a list's address
    return bl;
}

// The records carry addresses (low halves) of the window table at band_a and of the list table at rem_a.
static void pair_records(int N, int wpc, const RingGeometry &g, const std::vector<uint32_t> &rptr, uint64_t band_a, uint64_t rem_a,
                         std::vector<uint4> *rec)
{
    const int NB = 2 * g.NQ;
    rec->resize((size_t)N * wpc);
    for (int j = 0; j < N; ++j) {
        const int q0 = g.a4v[j] >> 7, lead = g.a4v[j] & 127;
        for (int w = 0; w < wpc; ++w) {
            int ph = (w - q0) % wpc; ph += ph < 0 ? wpc : 0;
            int gb = q0 + ph; gb -= gb >= NB ? NB : 0;
            const size_t q = (size_t)j * wpc + w;
            (*rec)[q] = lsm_lif::pair_record((uint32_t)(band_a + (uint64_t)j * g.pitch), (ph * 128 - lead) * 4, gb,
                                            (uint32_t)g.nbytes[j], (uint32_t)(rem_a + (uint64_t)rptr[q] * 8u), rptr[q + 1] - rptr[q]);
        }
    }
}

// Host-only (no GPU, no HIP call): the ring-window table, the pair-block lists and the row records lsm_reservoir_create would
// build for these CSC arrays and `wpc` waves per clip, with the tables placed at the given (fictitious) addresses.  Sizes first
// (null outputs), then the arrays.  Returns the blocks per wave, 0 when the reservoir has no pair layout with that many waves,
// < 0 on a bad argument.  tests/test_pair_layout.py applies every row from these tables alone and compares with the column.
extern "C" __attribute__((visibility("default")))
int lsm_debug_pair_layout(int num_neurons, const int32_t *csc_ptr, const int32_t *csc_post, const float *csc_w, int wpc,
                          unsigned long long band_addr, unsigned long long rem_addr, long *band_floats, long *n_list_entries,
                          int *pitch_bytes, float *band_out, uint32_t *rem_out, uint32_t *rec_out)
{
    LSM_REQUIRE(num_neurons >= 1 && num_neurons <= 8192 && csc_ptr && csc_post && csc_w, "lsm_debug_pair_layout: bad argument");
    LSM_REQUIRE(wpc == 4 || wpc == 8 || wpc == 16, "lsm_debug_pair_layout: wpc must be 4, 8 or 16");
    Network net;
    net.N = num_neurons; net.csc_ptr = csc_ptr; net.csc_post = csc_post; net.csc_w = csc_w; net.nnz = (size_t)csc_ptr[net.N];
    RingGeometry g;
    if (!ring_geometry(net, &g)) return 0;
    std::vector<uint32_t> rptr;
    std::vector<uint2> rem;
    const int bl = pair_lists(net, wpc, g, &rptr, &rem);
    if (!bl) return 0;
    if (band_floats) *band_floats = (long)net.N * (g.pitch / 4);
    if (n_list_entries) *n_list_entries = (long)rptr.back();
    if (pitch_bytes) *pitch_bytes = (int)g.pitch;
    if (band_out) {
        std::vector<float> band;
        ring_windows(net, g, &band);
        std::memcpy(band_out, band.data(), band.size() * sizeof(float));
    }
    if (rem_out) std::memcpy(rem_out, rem.data(), (size_t)rptr.back() * sizeof(uint2));
    if (rec_out) {
        std::vector<uint4> rec;
        pair_records(net.N, wpc, g, rptr, band_addr, rem_addr, &rec);
        std::memcpy(rec_out, rec.data(), rec.size() * sizeof(uint4));
    }
    return bl;
}

// The pair-block kernel's four input words per neuron (lif_pair.h), (npad, 4) in neuron order, for channels at the positions
// net.perm (coloured) or at their natural ones.  Returns the kernel's INMASK form: 1 = channel masks at the natural positions
// (C <= 128, no colouring), 2 = masks at coloured positions (C <= 128), 3 = {posmask, P0, P1, P2} over coloured positions
// (129..256 channels: bit p of posmask = a channel of colour p feeds the neuron, bit p of Pj = bit j of that channel's
// word), 0 = no such form: more than 256 channels, more than 128 without a colouring, or a channel that names a neuron
// twice (the words hold one bit per (channel, neuron) pair).  Host arithmetic only.
static int pair_input_words(const Network &net, int npad, std::vector<uint32_t> *im)
{
    if (net.C > 256 || (net.C > 128 && !net.perm)) return 0;
    if (net.C <= 128) return channel_masks(net, npad, im) ? (net.perm ? 2 : 1) : 0;
    im->assign((size_t)npad * 4, 0u);
    for (int c = 0; c < net.C; ++c)
        for (int d = 0; d < net.in_fanout; ++d) {
            const int pc = net.perm[c];
            const uint32_t bit = 1u << (pc & 31);
            uint32_t *m = im->data() + (size_t)net.in_tgt[(size_t)c * net.in_fanout + d] * 4;
            // channels that share a neuron differ in colour: a bit met twice is the SAME channel naming the neuron again
            if (m[0] & bit) return 0;
            m[0] |= bit;
            for (int j = 0; j < 3; ++j)
                if (((pc >> 5) >> j) & 1) m[1 + j] |= bit;
        }
    return 3;
}

// Host-only (no GPU, no HIP call): the channel positions (perm_out[n_channels]; the identity where the masks keep the natural
// positions) and the per-neuron input words (words_out[4 * NPAD], NPAD = 256 * ceil(num_neurons / 256)) lsm_reservoir_create
// would upload for the pair-block kernel with `wpc` (4, 8, 16) waves per clip.  Either output may be null.  Returns the
// input form (pair_input_words: 1, 2 or 3), 0 when the map has none or the blocks do not divide into 1..4 for each of `wpc`
// waves, < 0 on a bad argument.  tests/test_pair_inputs_host.py decodes the words back into the map, on the CPU.
extern "C" __attribute__((visibility("default")))
int lsm_debug_pair_inputs(int num_neurons, int n_channels, const int32_t *in_tgt, int in_fanout, int wpc, uint8_t *perm_out,
                          uint32_t *words_out)
{
    LSM_REQUIRE(num_neurons >= 1 && num_neurons <= 8192 && n_channels >= 1 && n_channels <= 65535 && in_tgt &&
                in_fanout >= 1 && in_fanout <= num_neurons, "lsm_debug_pair_inputs: bad argument");
    LSM_REQUIRE(wpc == 4 || wpc == 8 || wpc == 16, "lsm_debug_pair_inputs: wpc must be 4, 8 or 16");
    Network net;
    net.N = num_neurons; net.C = n_channels; net.in_tgt = in_tgt; net.in_fanout = in_fanout;
    for (size_t e = 0; e < (size_t)net.C * in_fanout; ++e)
        LSM_REQUIRE(in_tgt[e] >= 0 && in_tgt[e] < net.N, "lsm_debug_pair_inputs: in_tgt[%zu] out of range", e);
    const int NQ = (net.N + 255) / 256;
    if (!pair_blocks_per_wave(NQ, wpc)) return 0;
    std::vector<uint8_t> inperm;
    if (colour_input_channels(net.N, net.C, in_tgt, in_fanout, &inperm)) net.perm = inperm.data();
    std::vector<uint32_t> im;
    const int form = pair_input_words(net, NQ * 256, &im);
    if (!form) return 0;
    if (perm_out)
        for (int c = 0; c < net.C; ++c) perm_out[c] = net.perm ? net.perm[c] : (uint8_t)c;
    if (words_out) std::memcpy(words_out, im.data(), im.size() * sizeof(uint32_t));
    return form;
}

static int check_network(const Network &net, float theta, int refractory)
{
    const int N = net.N, C = net.C;
    // 8192: beyond that the per-clip LDS image (counts, spike lists, features, input bits) of neither kernel
    // fits the 160 KB of a CU
    LSM_REQUIRE(N >= 1 && N <= 8192, "num_neurons=%d outside [1, 8192]", N);
    LSM_REQUIRE(C >= 1 && C <= 65535, "n_channels=%d outside [1, 65535]", C);
    LSM_REQUIRE(net.n_out >= 1 && net.n_out <= N, "num_output_neurons=%d outside [1, %d]", net.n_out, N);
    LSM_REQUIRE(theta > 0.0f, "membrane_threshold must be > 0");
    LSM_REQUIRE(refractory >= 0 && net.in_fanout >= 1 && net.in_fanout <= N, "bad refractory/in_fanout");
    LSM_REQUIRE(net.csc_ptr && net.csc_post && net.csc_w && net.leak && net.in_tgt && net.out_idx, "null array argument");
    LSM_REQUIRE(net.csc_ptr[0] == 0, "csc_ptr[0] must be 0");
    for (int j = 0; j < N; ++j) {
        LSM_REQUIRE(net.csc_ptr[j + 1] >= net.csc_ptr[j], "csc_ptr not monotone at %d", j);
        for (int e = net.csc_ptr[j]; e < net.csc_ptr[j + 1]; ++e) {
            LSM_REQUIRE(net.csc_post[e] >= 0 && net.csc_post[e] < N, "csc_post[%d] out of range", e);
            LSM_REQUIRE(e == net.csc_ptr[j] || net.csc_post[e] > net.csc_post[e - 1],
                        "csc_post not strictly ascending within column %d", j);
        }
    }
    for (int o = 0; o < net.n_out; ++o)
        LSM_REQUIRE(net.out_idx[o] >= 0 && net.out_idx[o] < N && (o == 0 || net.out_idx[o] > net.out_idx[o - 1]),
                    "out_idx must be strictly ascending in [0, N)");
    for (int e = 0; e < C * net.in_fanout; ++e)
        LSM_REQUIRE(net.in_tgt[e] >= 0 && net.in_tgt[e] < N, "in_tgt[%d] out of range", e);
    return LSM_OK;
}

static int upload_csc(lsm_reservoir *h, const Network &net)
{
    std::vector<uint2> syn(net.nnz);
    for (size_t e = 0; e < net.nnz; ++e) syn[e] = make_uint2((uint32_t)net.csc_post[e], weight_bits(net.csc_w[e]));
    const int rc = upload(&h->syn, syn);
    if (rc) return rc;
    return upload(&h->rowptr, std::vector<uint32_t>(net.csc_ptr, net.csc_ptr + net.N + 1));
}

// Layout vi of the sparse and dense kernels: wpc = 1, 2, 4, 8, 16 waves per clip, wave w owning the neurons
// [w*sl*64, (w+1)*sl*64).  Left unavailable (wpc == 0) when a wave would own more than 16 slots of 64.
static int build_variant(lsm_reservoir *h, const Network &net, int vi)
{
    const int N = net.N, wpc = 1 << vi;
    const int need = ((N + wpc - 1) / wpc + 63) / 64;      // 64-neuron slots per wave
    int sl = 1;
    while (sl < need) sl <<= 1;
    if (sl > 16) return LSM_OK;
    const int npw = sl * 64, npad = npw * wpc;
    Variant &v = h->var[vi];
    // segment table: entry (j, w) = first synapse of column j whose target belongs to wave w;
    // the segment ends where entry (j, w+1) -- or column j+1 -- begins.
    std::vector<uint32_t> seg((size_t)N * wpc + 1);
    for (int j = 0; j < N; ++j) {
        int e = net.csc_ptr[j];
        for (int w = 0; w < wpc; ++w) {
            seg[(size_t)j * wpc + w] = (uint32_t)e;
            const int hi = (w + 1) * npw;
            while (e < net.csc_ptr[j + 1] && net.csc_post[e] < hi) ++e;
        }
    }
    seg[(size_t)N * wpc] = (uint32_t)net.nnz;
    // packed form for LDS: u16 offsets relative to the row start, WPC + 1 per neuron
    std::vector<uint16_t> segoff((size_t)N * (wpc + 1) + 2, 0);
    for (int j = 0; j < N; ++j) {
        for (int w = 0; w < wpc; ++w)
            segoff[(size_t)j * (wpc + 1) + w] = (uint16_t)(seg[(size_t)j * wpc + w] - (uint32_t)net.csc_ptr[j]);
        segoff[(size_t)j * (wpc + 1) + wpc] = (uint16_t)(net.csc_ptr[j + 1] - net.csc_ptr[j]);
    }
    std::vector<uint32_t> ent;              // (channel << 16) | target, whole rows of 64, 0xFFFFFFFF = padding
    const int einw = wave_entries(net, wpc, 64, [&](int i) { return i / npw; },
                                  [](int c, int i) { return ((uint32_t)c << 16) | (uint32_t)i; },
                                  [](size_t) { return 0xFFFFFFFFu; }, &ent);
    int rc;
    if ((rc = upload(&v.seg, seg)) || (rc = upload(&v.segoff, segoff)) || (rc = upload(&v.leak, padded_leak(net, npad))) ||
        (rc = upload(&v.oslot, output_slots(net, npad))) || (rc = upload(&v.in_ent, ent)))
        return rc;
    // INMODE 2 / 3 of the dense kernel: channel masks in registers
    if (net.C <= 128 && sl <= 4 && (rc = upload_channel_masks(net, npad, &v.inmask, &v.incol))) return rc;
    v.wpc = wpc; v.sl = sl; v.einw = einw;
    return LSM_OK;
}

// Layout vi of the ring-row kernel in quads (lif_ring.h): wpc = 2, 4, 8, 16 waves, contiguous (vi < 4) or strided quad
// ownership.  Left unavailable when the geometry does not allow it.
static int build_quads(lsm_reservoir *h, const Network &net, const RingGeometry &geo, int vi)
{
    const int N = net.N, wpc = 2 << (vi & 3);
    const bool strided = vi >= 4;
    int ql = 0;
    if (strided) {
        // every wave gets exactly one window quad per row: the residues mod wpc must survive the
        // ring's wrap (NQ % wpc == 0) and a window must not be wider than wpc quads
        if (geo.NQ % wpc != 0 || geo.wsq > wpc) return LSM_OK;
        ql = geo.NQ / wpc;
        if (ql < 1 || ql > 4) return LSM_OK;
    } else {
        for (int cand : {1, 2, 3, 4})
            if (!ql && wpc * cand * 256 >= N) ql = cand;
        // a wave must never hold both ends of a (wrapped) window: window quads + QL <= NQ
        if (!ql || geo.wsq + ql > geo.NQ) return LSM_OK;
    }
    const int npad = wpc * ql * 256;
    auto wave_of = [&](int i) { return lsm_lif::ring_wave_of_quad(i >> 8, ql, wpc, strided); };
    std::vector<uint32_t> rptr;
    std::vector<uint2> rem;
    const int emax = outside_lists(net, wpc, geo, wave_of, [](int i) { return (uint32_t)lsm_lif::ring_acc_word(i) * 4u; },
                                   &rptr, &rem);
    if (emax > 64) return LSM_OK;                            // one lane per list entry
    if (rptr.back() >= (1u << 24)) return LSM_OK;            // the kernel packs a list's start into 24 bits
    // input map per owner wave, packed (lsm_lif::ring_pack_entry), padded to whole blocks of RING_ENT_BLOCK so that the
    // kernel's drive needs no guards.  Padding entry at index e: channel 0 into dump word e % 64 -- every lane its OWN dump
    // word (64 lanes adding to one LDS word serialise: zero-padding cost cfg4 5 ms, profiles/r04_ring_input_drive.txt)
    std::vector<uint32_t> ent;
    const int einw = wave_entries(net, wpc, lsm_lif::RING_ENT_BLOCK, wave_of,
                                  [](int c, int i) { return lsm_lif::ring_pack_entry(c, i); },
                                  [](size_t e) { return (uint32_t)((e % 64) * 4); }, &ent);
    RingVariant &v = h->rvar[vi];
    int rc;
    if ((rc = upload(&v.rem_ptr, rptr)) || (rc = upload(&v.rem, rem)) || (rc = upload(&v.leak, padded_leak(net, npad))) ||
        (rc = upload(&v.oslot, output_slots(net, npad))) || (rc = upload(&v.in_ent, ent)))
        return rc;
    // INMASK form of the kernel (lif_ring.h): per-neuron channel masks in registers instead of the entry drive
    if (net.C <= 128 && h->leak_uniform && strided && ql <= 2 && (rc = upload_channel_masks(net, npad, &v.inmask, &v.incol)))
        return rc;
    v.wpc = wpc; v.ql = ql; v.einw = einw; v.strided = strided; v.n_rem = rptr.back();
    return LSM_OK;
}

// Layout vi of the ring-row kernel in pair blocks (lif_pair.h): wpc = 4, 8, 16 waves (pair_lists).  The kernel counts the
// input drive from four registers per neuron only: `im` in the form `inform` (pair_input_words).
static int build_pairs(lsm_reservoir *h, const Network &net, const RingGeometry &geo, int vi, int inform,
                       const std::vector<uint32_t> &im)
{
    const int N = net.N, wpc = 4 << vi, npad = geo.NQ * 256;
    std::vector<uint32_t> rptr;
    std::vector<uint2> rem;
    const int bl = pair_lists(net, wpc, geo, &rptr, &rem);
    if (!bl) return LSM_OK;
    // the records carry device addresses (low halves): upload the lists first; a table that crosses a 4 GB
    // line (the kernel takes the high address bits from the table pointer) cannot serve this layout
    PairVariant &v = h->pvar[vi];
    int rc;
    if ((rc = upload(&v.rem, rem))) return rc;
    const uint64_t band_a = reinterpret_cast<uint64_t>(h->band.get()), rem_a = reinterpret_cast<uint64_t>(v.rem.get());
    if ((band_a >> 32) != ((band_a + (uint64_t)N * geo.pitch) >> 32) ||
        (rem_a >> 32) != ((rem_a + (uint64_t)rem.size() * 8u) >> 32)) {
        v.rem.reset();
        return LSM_OK;
    }
    std::vector<uint4> rec;
    pair_records(N, wpc, geo, rptr, band_a, rem_a, &rec);
    if ((rc = upload(&v.rec, rec)) || (rc = upload(&v.oslot, output_slots(net, npad))) || (rc = upload(&v.inmask, im)))
        return rc;
    // a coefficient per neuron (LEAKV form of the kernel)
    if (!h->leak_uniform && (rc = upload(&v.leak, padded_leak(net, npad)))) return rc;
    v.inform = inform;
    v.wpc = wpc; v.bl = bl; v.n_rem = rptr.back();
    return LSM_OK;
}

// Dense rows at creation, unless auto mode will serve this reservoir with ring rows: the table exceeds the L2 caches, ring
// rows exist AND one of their layouts fits a CU's LDS with room to spare (probed at 1024 time steps; the
// reference runs 400).  Then the 64-262 MB table and its upload would be dead weight next to the ring table
// (ADVICE r2); lsm_reservoir_set_kernel(2) still builds it on request.  When no ring layout fits (e.g. N = 8000
// with 5000 output neurons) the dense kernel is auto mode's fallback and needs its table from the start.
static bool ring_serves_auto(const lsm_reservoir *h)
{
    if (!has_ring(h) || (size_t)h->N * (size_t)h->ld * 4 <= RING_AUTO_MIN_DENSE_BYTES) return false;
    // (a pair-block layout implies strided quad layouts of the same table exist; the quads decide)
    for (const auto &v : h->rvar)
        if (v.wpc && ring_lds_bytes(h, v, 1024) <= 160 * 1024) return true;
    return false;
}

// Any refractory period >= 0 is accepted and stored as min(refractory, 65535): a run has at most 65535 steps, so a neuron
// that fires at step t is held through the end of the clip either way -- the same simulation -- and the ring and pair kernels
// keep the countdown in the upper 16 bits of a register (lif_ring.h, lif_pair.h).  An input map may name a neuron more than
// once in one channel (every entry counts); such a map has no channel-mask or bit-plane form, hence no pair-block layout.
extern "C" __attribute__((visibility("default")))
int lsm_reservoir_create(lsm_reservoir **out, int num_neurons, int n_channels,
                         const int32_t *csc_ptr, const int32_t *csc_post, const float *csc_w,
                         const float *leak, const int32_t *in_tgt, int in_fanout, float w_in,
                         const int32_t *out_idx, int n_out, float theta, int refractory,
                         int burst_isi_max)
{
    LSM_REQUIRE(out != nullptr, "lsm_reservoir_create: out is null");
    *out = nullptr;
    Network net;
    net.N = num_neurons; net.C = n_channels; net.csc_ptr = csc_ptr; net.csc_post = csc_post; net.csc_w = csc_w;
    net.leak = leak; net.in_tgt = in_tgt; net.in_fanout = in_fanout; net.out_idx = out_idx; net.n_out = n_out;
    int rc = check_network(net, theta, refractory);
    if (rc) return rc;
    const int N = net.N;
    net.nnz = (size_t)csc_ptr[N];

    std::unique_ptr<lsm_reservoir> h(new lsm_reservoir());
    h->N = N; h->C = net.C; h->n_out = n_out; h->refractory = std::min(refractory, 65535);
    h->burst_isi_max = burst_isi_max; h->theta = theta; h->w_in = w_in; h->nnz = net.nnz;
    (void)hipGetDevice(&h->device);
    if (hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) {
        (void)hipGetLastError();
        h->cus = 0;
    }
    if ((rc = upload_csc(h.get(), net))) return rc;

    // coloured bit positions for the input masks of the dense kernel and the pair blocks (one assignment per reservoir)
    std::vector<uint8_t> inperm;
    if (colour_input_channels(N, net.C, in_tgt, in_fanout, &inperm)) {
        net.perm = inperm.data();
        if ((rc = upload(&h->inperm, inperm))) return rc;
    }
    h->leak_uniform = true;
    h->leak_u = leak[0];
    for (int i = 1; i < N; ++i)
        if (std::memcmp(&leak[i], &leak[0], sizeof(float)) != 0) { h->leak_uniform = false; break; }

    for (int vi = 0; vi < 5; ++vi)
        if ((rc = build_variant(h.get(), net, vi))) return rc;
    // dense presynaptic rows for the register-accumulating kernel (lif_dense.h): N x ld floats (4 MB at N = 1000:
    // L2; 64 MB at N = 4000 and 262 MB at N = 8000).  Built at the end, and only when auto mode can run them
    // (ring_serves_auto); a reservoir that auto mode serves with ring rows gets them on lsm_reservoir_set_kernel(2).
    for (const auto &v : h->var)
        if (v.wpc) h->ld = std::max(h->ld, v.sl * 64 * v.wpc);

    // Ring rows for ring-like graphs (lif_ring.h, lif_pair.h).  (The ring kernel counts a neuron's active input entries of
    // a step in 16 bits.)
    std::vector<uint32_t> fanin(N, 0u);
    uint32_t max_fanin = 0;
    for (size_t e = 0; e < (size_t)net.C * in_fanout; ++e) max_fanin = std::max(max_fanin, ++fanin[in_tgt[e]]);
    RingGeometry geo;
    if (max_fanin <= 65535u && ring_geometry(net, &geo)) {
        std::vector<float> band;
        ring_windows(net, geo, &band);
        if ((rc = upload(&h->band, band))) return rc;
        h->band_pitch = geo.pitch; h->band_h = geo.H; h->band_nq = geo.NQ; h->band_wsq = geo.wsq;
        for (int j = 0; j < N; ++j) h->band_bytes_sum += geo.nbytes[j];
        for (int vi = 0; vi < 8; ++vi)
            if ((rc = build_quads(h.get(), net, geo, vi))) return rc;
        std::vector<uint32_t> im;
        const int inform = pair_input_words(net, geo.NQ * 256, &im);
        for (int vi = 0; vi < 3 && inform != 0; ++vi)
            if ((rc = build_pairs(h.get(), net, geo, vi, inform, im))) return rc;
    }
    if (!ring_serves_auto(h.get()) && (rc = ensure_dense_rows(h.get()))) return rc;
    *out = h.release();
    return LSM_OK;
}

// 0 = choose, 1 = sparse CSC kernel, 2 = dense-row kernel, 3 = ring-row kernel.
extern "C" __attribute__((visibility("default")))
int lsm_reservoir_set_kernel(lsm_reservoir *h, int mode)
{
    LSM_REQUIRE(h != nullptr, "lsm_reservoir_set_kernel: null handle");
    LSM_REQUIRE(mode >= MODE_AUTO && mode <= MODE_RING_QUADS, "mode must be 0 (auto), 1 (sparse), 2 (dense), 3 (ring), 4 (ring, contiguous quads), "
                "5 (ring, pair blocks) or 6 (ring, quads)");
    LSM_REQUIRE(mode < MODE_RING || has_ring(h), "this reservoir has no ring-row format (not ring-like, or too small)");
    LSM_REQUIRE(mode != MODE_RING_PAIRS || has_pairs(h), "this reservoir has no pair-block ring layout (needs at most 256 channels -- above 128 "
                "with bit positions in which the channels feeding one neuron differ mod 32, so at most 32 channels per neuron --, "
                "an input map that names no neuron twice in one channel, a block count that is a multiple of 4, 8 or 16 waves and "
                "a window of at most that many blocks)");
    if (mode == MODE_DENSE) {                       // an explicit request builds the table a ring-served reservoir deferred
        const int rc = ensure_dense_rows(h);
        if (rc) return rc;
        LSM_REQUIRE(h->wt != nullptr, "this reservoir has no dense row table");
    }
    h->mode = static_cast<KernelMode>(mode);
    return LSM_OK;
}

extern "C" __attribute__((visibility("default")))
int lsm_reservoir_destroy(lsm_reservoir *h)
{
    delete h;
    return LSM_OK;
}

static bool lif_inreg(const Variant &v) { return v.einw <= IN_REG_SLOTS * 64; }

static bool ring_inreg(const RingVariant &rv)
{
    // the wave's input map stays in registers when it is one block (8 registers) AND the layout has few neurons per
    // lane: with three or four quads per wave the extra registers would cost a wave per SIMD
    return rv.einw <= lsm_lif::RING_ENT_BLOCK * lsm_lif::RING_ENT_REG_BLOCKS && rv.ql <= 2 && rv.strided;
}

// words of a step's input bit row
static size_t input_words(const lsm_reservoir *h) { return (size_t)(h->C + 31) / 32; }

// What every kernel keeps in LDS behind its own arrays: the feature accumulators and the clip's input bits.
static size_t lds_tail_bytes(const lsm_reservoir *h, int T) { return (size_t)h->n_out * 16 + (size_t)T * input_words(h) * 4; }

static size_t lif_lds_core(const lsm_reservoir *h, const Variant &v, int T)
{
    const size_t npad = (size_t)v.sl * 64 * v.wpc;
    return npad * 4 + npad * 4 + 2 * npad * 2 + 128 + lds_tail_bytes(h, T);
}

static size_t lif_seg_bytes(const lsm_reservoir *h, const Variant &v)
{
    // packed LDS form: (N+1) u32 row pointers + N*(WPC+1) u16 offsets (rounded up to a whole dword)
    return ((size_t)h->N + 1) * 4 + (((size_t)h->N * (v.wpc + 1) + 1) / 2) * 4;
}

// The segment table rides in LDS when that still leaves room for >= 2 workgroups per CU's 160 KB.
static bool lif_seg_in_lds(const lsm_reservoir *h, const Variant &v, int T)
{
    return lif_lds_core(h, v, T) + lif_seg_bytes(h, v) <= 80 * 1024;
}

static size_t lif_lds_bytes(const lsm_reservoir *h, const Variant &v, int T)
{
    return lif_lds_core(h, v, T) + (lif_seg_in_lds(h, v, T) ? lif_seg_bytes(h, v) : 0);
}

static size_t ring_lds_bytes(const lsm_reservoir *h, const RingVariant &v, int T)
{
    const size_t npad = (size_t)v.ql * 256 * v.wpc;
    // float32 accumulators + 16-bit input counts (each behind 64 dump words; no counts when the kernel counts from
    // per-neuron masks, INMASK), two step lists, quad counts, feature accumulators, the clip's input bits
    const size_t cnt_words = v.inmask ? 0 : (size_t)lsm_lif::RING_DUMP_WORDS + npad / 2;
    return ((size_t)lsm_lif::RING_DUMP_WORDS + npad + cnt_words) * 4 +
           2 * npad * 2 + 512 + lds_tail_bytes(h, T);
}

static size_t pair_lds_bytes(const lsm_reservoir *h, const PairVariant &v, int T)
{
    const size_t npad = (size_t)v.bl * 128 * v.wpc;
    // dump words, float32 accumulators, 64 scratch words per wave, two step lists of bytes, block counts, feature
    // accumulators, the clip's input bits
    return (size_t)lsm_lif::PAIR_DUMP_BYTES + npad * 4 + (size_t)v.wpc * 256 + 2 * npad +
           (size_t)lsm_lif::PAIR_WCNT_WORDS * 4 + lds_tail_bytes(h, T);
}

// Static LDS bytes of a pair-block kernel, asked once per kernel for the life of the process.  lif_pair.h addresses LDS
// by absolute byte address, which holds only while the kernel has no static LDS (its dynamic LDS then starts at 0).
static int pair_static_lds(const void *fn, size_t *bytes)
{
    static std::mutex mu;
    static std::map<const void *, size_t> known;
    std::lock_guard<std::mutex> lk(mu);
    auto it = known.find(fn);
    if (it == known.end()) {
        hipFuncAttributes fa;
        LSM_CHECK_HIP(hipFuncGetAttributes(&fa, fn));
        it = known.emplace(fn, fa.sharedSizeBytes).first;
    }
    *bytes = it->second;
    return LSM_OK;
}

// Whether auto and "ring" take the bit-plane form of the pair blocks (129..256 channels) where the rule below allows it.
// The form has not been timed against the quads yet (profiles/pair_wide_channels.txt: the comparison exp/pair_wide_channels.py
// makes is not on record), and the default changes only on a measured gain beyond the run-to-run spread: until then such
// reservoirs keep the kernel they had, and the pair blocks are there by name (mode 5).
constexpr bool PAIR_WIDE_AUTO = false;

// Pair-block layout for a batch: the requested waves per clip, else the fewest waves (every wave repeats the per-row work).
static const PairVariant *choose_pair(const lsm_reservoir *h, int T, int requested)
{
    if (h->mode != MODE_AUTO && h->mode != MODE_RING && h->mode != MODE_RING_PAIRS) return nullptr;
    for (const auto &v : h->pvar) {
        if (!v.wpc || pair_lds_bytes(h, v, T) > 160 * 1024) continue;
        if (requested > 0 && v.wpc != requested) continue;
        // Unless pair blocks are asked for by name, they are taken where they pay: with at least three blocks per wave.
        // Same box, 512 clips, k = 0.2 N (profiles/r05_midsize_pairs_vs_quads.txt): N = 1536 (3 blocks, 4 waves) 1.33 ms
        // against 2.95 in quads, N = 4000 (4 blocks) 4.17 against 5.10, N = 3072 (3 blocks, 8 waves) 3.47 against 3.45 --
        // but N = 2048 (2 blocks, 8 waves) 2.46 against 2.19: with few neurons per lane the per-wave work per row dominates
        // and the quads' four fat waves win.
        if (h->mode != MODE_RING_PAIRS && v.bl < 3 && has_ring(h)) continue;
        // Above 128 channels (bit planes, inform 3): by name only while PAIR_WIDE_AUTO is off, and never by default where the
        // layout needs 16 waves (N = 8000 with 256 filters: the quads run at 99 % of the gather ceiling there, 16 waves repeat
        // the per-row work of 8: N = 8000 strided quads, 8 waves 29.0 ms, 16 waves 36.8 ms).
        if (h->mode != MODE_RING_PAIRS && v.inform == 3 && (v.wpc == 16 || !PAIR_WIDE_AUTO)) continue;
        return &v;
    }
    return nullptr;
}

// Ring layout for a batch: the requested waves per clip, else a strided layout when the reservoir has one (every
// wave gets one useful 1 KB window load per row: N=8000, 8 waves: 29.0 ms against 42.0 ms contiguous; N=4000:
// 8 waves strided 9.7 ms against 4 fat waves contiguous 10.2 ms), and within a kind the layout with the fewest
// waves that still gives a clip at least 4 (every wave repeats the per-row work -- list hand-off, row
// parameters: N=8000 strided, 8 waves 29.0 ms, 16 waves 36.8 ms; N=4000 contiguous, 4 waves 10.2 ms, 8 waves 13.9 ms).
static const RingVariant *choose_ring(const lsm_reservoir *h, int T, int requested)
{
    const RingVariant *best = nullptr;
    auto better = [](const RingVariant &v, const RingVariant &b) {
        if (v.strided != b.strided) return v.strided;
        const bool v4 = v.wpc >= 4, b4 = b.wpc >= 4;
        if (v4 != b4) return v4;
        return v4 ? v.wpc < b.wpc : v.wpc > b.wpc;
    };
    if (h->mode == MODE_RING_PAIRS) return nullptr;
    for (const auto &v : h->rvar) {
        if (!v.wpc || ring_lds_bytes(h, v, T) > 160 * 1024) continue;
        if (v.strided && h->mode == MODE_RING_CONTIGUOUS) continue;
        if (requested > 0 && v.wpc != requested) continue;
        if (!best || better(v, *best)) best = &v;
    }
    return best;
}

static bool want_ring(const lsm_reservoir *h)
{
    if (!has_ring(h)) return false;
    if (h->mode >= MODE_RING) return true;
    return h->mode == MODE_AUTO && (size_t)h->N * (size_t)h->ld * 4 > RING_AUTO_MIN_DENSE_BYTES;
}
static bool use_dense(const lsm_reservoir *h) { return h->wt != nullptr && h->mode != MODE_SPARSE; }

static size_t dense_lds_bytes(const lsm_reservoir *h, const Variant &v, int T)
{
    const size_t npad = (size_t)v.sl * 64 * v.wpc;
    return npad * 4 + 2 * npad * 2 + 512 + lds_tail_bytes(h, T);
}

// Pick the waves-per-clip layout.  Measured on MI355X at N=1000 (profiles/): the best layout has
// about 4096 wavefronts in flight (B=256 -> 16, B=512 -> 8) and never fewer than 4 waves per clip
// (B=4096: 4 waves 9.1 ms, 2 waves 10.6 ms, 1 wave 17.6 ms).  Among the layouts this reservoir
// supports and whose LDS image fits one CU, take the smallest one at or above that target.
// requested == -1: the launch runs inside an overlapped pipeline (other kernels share the CUs): the chip is
// then bound by vector-ALU issue and fewer, fatter waves spend fewer instructions on per-wave overheads
// (N=1000, B=256: 4 waves per clip 3.5 % faster for the whole pipeline than 8; a lone launch prefers 8).
static const Variant *choose_variant(const lsm_reservoir *h, int B, int T, int requested)
{
    // LDS image of the kernel that will run (the dense-row kernel needs less than the sparse one)
    auto lds_of = [&](const Variant &v) {
        return use_dense(h) ? dense_lds_bytes(h, v, T) : lif_lds_bytes(h, v, T);
    };
    if (requested > 0) {
        for (const auto &v : h->var)
            if (v.wpc == requested && lds_of(v) <= 160 * 1024) return &v;
        return nullptr;
    }
    int target = 4;
    // dense-row kernel (measured at N=1000, B=256: 4 waves 0.82 ms, 8 waves 0.75 ms, 16 waves 0.81 ms):
    // about 2048 wavefronts; sparse kernel: about 4096
    const long want = use_dense(h) ? 2048 : 4096;
    if (requested == 0)
        while (target < 16 && (long)B * target < want) target <<= 1;
    // large reservoirs: more waves per clip keep the per-lane neuron slots (registers, update work per
    // wave) small -- N=4000, B=1024: 4 waves 68 ms, 8 waves 43 ms, 16 waves 26 ms
    const Variant *best = nullptr;
    for (const auto &v : h->var) {
        if (!v.wpc || lds_of(v) > 160 * 1024) continue;
        if (!best || best->wpc < target || best->sl > 4) best = &v;
    }
    return best;
}

extern "C" __attribute__((visibility("default")))
long lsm_reservoir_order_workspace(int n_clips)
{
    return n_clips > 0 ? 2L * n_clips * (long)sizeof(int32_t) : 0L;     // spike count and start order of every clip
}

// ---- longest clips first (lsm_reservoir_run_ordered) --------------------------------------------------------------
// A clip's time in the LIF kernels grows with its activity (rows per step), and activity follows the input: at
// N = 4000 the input spike count of a clip predicts its reservoir spikes with a rank correlation of 0.99, and clips of
// one batch differ by a factor of 9.  A launch of several rounds (more clips than the chip holds at once) is then as
// long as the clip that happens to start last: 8.8 ms for 1024 clips whose work fills the chip for 5.1 ms.  Workgroups
// are dispatched in index order, so handing workgroup g the clip with the g-th most input spikes is the classic
// longest-processing-time-first schedule.  Results do not depend on it: every clip is simulated on its own.
// The non-zero bytes among the four of w: raster bytes are 0 or 1, and anything else counts as a spike in the LIF kernels too.
// (Per word, so that both key kernels keep adding the four counts of a 16-byte group straight into their sum.)
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w)
{
    uint32_t nz = w | (w >> 4);
    nz |= nz >> 2; nz |= nz >> 1;
    return __popc(nz & 0x01010101u);
}

__global__ __launch_bounds__(256) void clip_keys_kernel(const uint8_t *raster, long bytes_per_clip, int n_clips,
                                                        int32_t *keys)
{
    const int b = blockIdx.x;
    const uint8_t *clip = raster + (size_t)b * (size_t)bytes_per_clip;
    uint32_t sum = 0;
    long i = threadIdx.x * 16L;
    if ((reinterpret_cast<uintptr_t>(clip) & 15) == 0) {
        for (; i + 16 <= bytes_per_clip; i += 256 * 16L) {
            const uint4 v = *reinterpret_cast<const uint4 *>(clip + i);
            const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) sum += nonzero_bytes(w4[k]);
        }
        // the bytes behind the last full 16-byte group of the whole clip
        if (threadIdx.x == 0)
            for (long t = bytes_per_clip & ~15L; t < bytes_per_clip; ++t) sum += clip[t] != 0;
    } else {
        for (long t = threadIdx.x; t < bytes_per_clip; t += 256) sum += clip[t] != 0;
    }
    __shared__ uint32_t part[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor((int)sum, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) keys[b] = (int32_t)(part[0] + part[1] + part[2] + part[3]);
}

// The same key for a ragged launch (lsm_reservoir_run_ragged, SPEC.md §4c): clip b's non-zero bytes at t < L_b of every
// channel row, L_b = clip_steps[b] clamped into [0, n_steps] -- bytes behind a clip's length are neither read nor counted,
// and a clip of no steps gets key 0 and starts last.  One wave per channel row at a time (rows c = wave, wave + 4, ...):
// the row's valid prefix is read 16 bytes per lane from its first 16-byte-aligned address on, its head and tail by bytes.
// seg > 0 (stream launch, SPEC.md §4d): clip_steps counts whole segments of seg steps, L_b = clamp(clip_steps[b], 0,
// n_steps / seg) * seg -- the same arithmetic as clip_step_count (lif_common.h).
__global__ __launch_bounds__(256) void clip_keys_ragged_kernel(const uint8_t *raster, int n_channels, int n_steps,
                                                               const int32_t *clip_steps, int n_clips, int32_t *keys, int seg)
{
    const int b = blockIdx.x;
    const int len = seg > 0 ? min(max(clip_steps[b], 0), n_steps / seg) * seg
                            : min(max(clip_steps[b], 0), n_steps);      // workgroup-uniform
    const uint8_t *clip = raster + (size_t)b * (size_t)n_channels * (size_t)n_steps;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t sum = 0;
    for (int c = wave; c < n_channels; c += 4) {
        const uint8_t *row = clip + (size_t)c * (size_t)n_steps;
        // [0, head) and [body_end, len) by bytes, [head, body_end) in 16-byte groups
        const int head = min(len, (int)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u));
        const int body_end = head + ((len - head) & ~15);
        for (int t = head + lane * 16; t < body_end; t += 64 * 16) {
            const uint4 v = *reinterpret_cast<const uint4 *>(row + t);
            const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) sum += nonzero_bytes(w4[k]);
        }
        if (lane < head) sum += row[lane] != 0;                          // head < 16
        if (body_end + lane < len) sum += row[body_end + lane] != 0;     // len - body_end < 16
    }
    __shared__ uint32_t part[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor((int)sum, off, 64);
    if (lane == 0) part[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) keys[b] = (int32_t)(part[0] + part[1] + part[2] + part[3]);
}

constexpr int ORDER_WINDOW = 4096;      // clips ranked against each other (bounds the quadratic ranking)
static_assert(ORDER_WINDOW % 256 == 0, "a ranking workgroup stays inside one window");

// order[first + rank] = clip, rank = position of the clip in its window by (key descending, index ascending).
// A workgroup ranks 256 clips of one window; the window's keys pass through LDS in tiles of 1024, read back 16 bytes
// at a time at the same address in every lane (first version: every lane walked the keys in global memory, 63 us for
// 1024 clips -- 1 % of the cfg4 launch it schedules; now 28 us and less).
__global__ __launch_bounds__(256) void clip_rank_kernel(const int32_t *keys, int n_clips, int32_t *order)
{
    __shared__ __attribute__((aligned(16))) int32_t tile[1024];
    const int i = blockIdx.x * 256 + threadIdx.x;           // ORDER_WINDOW is a multiple of 256: a workgroup never straddles two windows
    const int first = (blockIdx.x * 256) / ORDER_WINDOW * ORDER_WINDOW;
    const int last = min(n_clips, first + ORDER_WINDOW);
    const bool mine = i < n_clips;
    const int32_t ki = mine ? keys[i] : 0;
    int rank = 0;
    for (int t0 = first; t0 < last; t0 += 1024) {
        __syncthreads();
        for (int q = threadIdx.x; q < 1024; q += 256) tile[q] = t0 + q < last ? keys[t0 + q] : INT32_MIN;
        __syncthreads();
        // INT32_MIN pads the tile: no key (a count >= 0) is smaller or equal, so padding never adds to a rank
        const int n4 = (min(1024, last - t0) + 3) / 4;
#pragma unroll 8
        for (int q = 0; q < n4; ++q) {
            const int4 k4 = reinterpret_cast<const int4 *>(tile)[q];
            const int j = t0 + 4 * q;
            rank += (k4.x > ki) || (k4.x == ki && j < i);
            rank += (k4.y > ki) || (k4.y == ki && j + 1 < i);
            rank += (k4.z > ki) || (k4.z == ki && j + 2 < i);
            rank += (k4.w > ki) || (k4.w == ki && j + 3 < i);
        }
    }
    if (mine) order[first + rank] = i;
}

// ONE decision for lsm_reservoir_run, lsm_reservoir_layout, lsm_reservoir_plan and lsm_reservoir_kernel_in_use:
// which kernel and which layout serve (handle, batch, steps, waves_per_clip).  Auto mode prefers ring rows for
// large ring-like reservoirs but FALLS THROUGH to the dense (else sparse) kernel when no ring layout fits -- the
// per-clip LDS image exceeds 160 KB (e.g. N = 8000 with 5000 output neurons: 175.7 KB as ring rows, 158.8 KB
// for the dense/sparse layouts) or the reservoir's ring layouts lack the requested waves per clip.
// Only an explicit ring request (MODE_RING and above) is a hard error then.
struct RunPlan {
    PlannedKernel kernel = KERNEL_NONE;
    const PairVariant *pv = nullptr;  // ring rows in pair blocks (lif_pair.h) when set, else
    const RingVariant *rv = nullptr;
    const Variant *v = nullptr;
};

static int make_plan(const lsm_reservoir *h, int n_clips, int n_steps, int waves_per_clip, RunPlan *p)
{
    if (want_ring(h)) {
        // pair blocks where the reservoir has them (cfg4: 5.1 -> see profiles/r05_*), else quads
        p->pv = choose_pair(h, n_steps, waves_per_clip > 0 ? waves_per_clip : 0);
        if (p->pv) { p->kernel = KERNEL_RING; return LSM_OK; }
        p->rv = choose_ring(h, n_steps, waves_per_clip > 0 ? waves_per_clip : 0);
        if (p->rv) { p->kernel = KERNEL_RING; return LSM_OK; }
        LSM_REQUIRE(h->mode < MODE_RING, "no ring-row layout for waves_per_clip=%d (N=%d, n_out=%d, T=%d): none fits a CU's "
                    "160 KB of LDS or has that many waves", waves_per_clip, h->N, h->n_out, n_steps);
    }
    p->v = choose_variant(h, n_clips, n_steps, waves_per_clip);
    LSM_REQUIRE(p->v != nullptr, "no reservoir layout for waves_per_clip=%d (N=%d, n_out=%d, T=%d)",
                waves_per_clip, h->N, h->n_out, n_steps);
    p->kernel = use_dense(h) ? KERNEL_DENSE : KERNEL_SPARSE;
    return LSM_OK;
}

// One launch: every run export fills its members by name, reservoir_run and the launch functions below read them.  The four
// flags say which refusals apply (check_run); which kernel forms run follows from the values (stateful, set_common_args).
struct RunArgs {
    const uint8_t *raster = nullptr;
    int n_clips = 0, n_steps = 0, n_keys = 0;
    const int32_t *key_ids = nullptr;
    float *features = nullptr, *v_trace = nullptr;
    uint8_t *spike_matrix = nullptr;
    int32_t *stats = nullptr;
    int waves_per_clip = 0;
    // longest clips first: the caller's workspace (lsm_reservoir_order_workspace), or null: clips start in index order.
    // order_clips fills `order`, the clip of workgroup g, when the launch has more workgroups than the chip has CUs.
    void *workspace = nullptr;
    long workspace_bytes = 0;
    const int32_t *order = nullptr;
    void *stream = nullptr;
    // continuation (`from`: lsm_reservoir_run_from and every export after it): the state blocks read / written and the
    // steps done before this launch.  Either pointer set selects the kernels' ST forms; lsm_reservoir_run and _run_ordered
    // leave them null, and a run_from call with neither is lsm_reservoir_run.
    bool from = false;
    const void *state_in = nullptr;
    void *state_out = nullptr;
    int first_step = 0;
    // segments (`segmented`: lsm_reservoir_run_segments, _run_stream): steps per segment and the records buffer; the ST
    // forms close the records
    bool segmented = false;
    int segment_steps = 0;
    void *records = nullptr;
    // ragged launch (lsm_reservoir_run_ragged, SPEC.md §4c): device array of the steps every clip runs, or null: n_steps.
    // The entry always takes the ST forms (`ragged`), with or without lengths.
    const int32_t *clip_steps = nullptr;
    bool ragged = false;
    // stream launch (lsm_reservoir_run_stream, SPEC.md §4d): segmented, clip_steps counts whole segments, no cumulative record
    bool streamed = false;
    bool stateful() const
    {
        return state_in != nullptr || state_out != nullptr || segment_steps > 0 || clip_steps != nullptr || ragged;
    }
};

// The fields LifArgs, DenseArgs, RingArgs and PairArgs have in common.
template <typename Args>
static void set_common_args(Args *a, const lsm_reservoir *h, const RunArgs &r)
{
    a->N = h->N; a->C = h->C; a->T = r.n_steps; a->B = r.n_clips;
    a->n_out = h->n_out; a->CW = (int)input_words(h);
    a->refractory = h->refractory; a->burst_isi_max = h->burst_isi_max;
    a->theta = h->theta; a->w_in = h->w_in;
    a->raster = r.raster;
    a->n_keys = r.n_keys;
    for (int k = 0; k < 8; ++k) a->key_ids[k] = k < r.n_keys ? r.key_ids[k] : 0;
    a->features = r.features; a->spike_matrix = r.spike_matrix; a->v_trace = r.v_trace;
    a->stats = r.stats; a->order = r.order;
    a->st.in = static_cast<const unsigned char *>(r.state_in); a->st.out = static_cast<unsigned char *>(r.state_out);
    a->st.stride = lsm_lif::state_bytes(h->N, h->n_out); a->st.t0 = r.streamed ? lsm_lif::STREAM_T0 : r.first_step;
    a->st.seg = r.segment_steps; a->st.rec = static_cast<uint4 *>(r.records);
    a->st.steps = r.clip_steps; a->st.count_limit = r.streamed ? r.n_steps / r.segment_steps : r.n_steps;
    a->st.count_steps = r.streamed ? r.segment_steps : 1;
}

// One workgroup of wpc waves per clip, `lds` bytes of dynamic LDS.
template <typename Args>
static int launch(void (*fn)(const Args), const Args &a, const RunArgs &r, int wpc, size_t lds)
{
    if (lds > 64 * 1024) lsm_allow_big_lds(reinterpret_cast<const void *>(fn));
    hipLaunchKernelGGL(fn, dim3(r.n_clips), dim3(wpc * 64), lds, (hipStream_t)r.stream, a);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

static int run_pairs(const lsm_reservoir *h, const PairVariant &pv, const RunArgs &r)
{
    const int inmask = pv.inform;
    const bool leakv = pv.leak != nullptr;
    static lsm_lif::pair_fn_t (*const wide[4])(int, bool, bool) = {lsm_lif::pick_pair_wide_1, lsm_lif::pick_pair_wide_2,
                                                             lsm_lif::pick_pair_wide_3, lsm_lif::pick_pair_wide_4};
    static lsm_lif::pair_fn_t (*const masks[4])(int, int, bool, bool) = {lsm_lif::pick_pair_1, lsm_lif::pick_pair_2,
                                                                   lsm_lif::pick_pair_3, lsm_lif::pick_pair_4};
    const bool st = r.stateful();
    lsm_lif::pair_fn_t pfn = inmask == 3 ? wide[pv.bl - 1](pv.wpc, leakv, st) : masks[pv.bl - 1](pv.wpc, inmask, leakv, st);
    // (bit planes: 5..8 row words, and the whole input image is T * cw words -- pair_lds_bytes)
    const size_t cw = input_words(h);
    LSM_REQUIRE(inmask != 3 || (cw >= 5 && cw <= 8), "pair-block bit planes with %zu row words", cw);
    LSM_REQUIRE(pfn != nullptr, "no pair-block ring kernel for BL=%d WPC=%d", pv.bl, pv.wpc);
    size_t static_lds = 0;
    const int src = pair_static_lds(reinterpret_cast<const void *>(pfn), &static_lds);
    if (src != LSM_OK) return src;
    if (static_lds != 0) {
        lsm_set_error("pair-block ring kernel BL=%d WPC=%d has %zu bytes of static LDS: its row loop addresses LDS "
                      "absolutely and needs its dynamic LDS to start at byte 0 (defective build)", pv.bl, pv.wpc,
                      static_lds);
        return LSM_ERR_UNSUPPORTED;
    }
    lsm_lif::PairArgs a;
    set_common_args(&a, h, r);
    a.leak_u = h->leak_u;
    a.band = h->band.get(); a.rec = pv.rec.get(); a.rem = pv.rem.get();
    a.oslot = pv.oslot.get(); a.leak = pv.leak.get(); a.inmask = pv.inmask.get();
    a.inperm = pv.inform >= 2 ? h->inperm.get() : nullptr;
    return launch(pfn, a, r, pv.wpc, pair_lds_bytes(h, pv, r.n_steps));
}

static int run_quads(const lsm_reservoir *h, const RingVariant &rv, const RunArgs &r)
{
    const bool inreg = ring_inreg(rv);
    const bool inmask = rv.inmask != nullptr;
    const bool st = r.stateful();
    lsm_lif::ring_fn_t rfn = inmask ? (rv.ql == 1 ? lsm_lif::pick_ring_mask_1(rv.wpc, rv.incol ? 2 : 1, st)
                                                  : lsm_lif::pick_ring_mask_2(rv.wpc, rv.incol ? 2 : 1, st))
                             : rv.ql == 1 ? lsm_lif::pick_ring_1(rv.wpc, inreg, rv.strided, st)
                             : rv.ql == 2 ? lsm_lif::pick_ring_2(rv.wpc, inreg, rv.strided, st)
                             : rv.ql == 3 ? lsm_lif::pick_ring_3(rv.wpc, inreg, rv.strided, st)
                                          : lsm_lif::pick_ring_4(rv.wpc, inreg, rv.strided, st);
    LSM_REQUIRE(rfn != nullptr, "no ring kernel for QL=%d WPC=%d", rv.ql, rv.wpc);
    lsm_lif::RingArgs a;
    set_common_args(&a, h, r);
    a.EinW = rv.einw;
    a.H = h->band_h; a.NQ = h->band_nq; a.pitch = h->band_pitch;
    a.band = h->band.get(); a.rem_ptr = rv.rem_ptr.get(); a.rem = rv.rem.get();
    a.leak = rv.leak.get(); a.oslot = rv.oslot.get(); a.in_ent = rv.in_ent.get();
    a.inmask = rv.inmask.get(); a.inperm = (inmask && rv.incol) ? h->inperm.get() : nullptr; a.leak_u = h->leak_u;
    return launch(rfn, a, r, rv.wpc, ring_lds_bytes(h, rv, r.n_steps));
}

static int run_dense(const lsm_reservoir *h, const Variant &v, const RunArgs &r)
{
    // the reference's refractory period (2 steps) counts down in scalar lane masks (lif_dense.h, REFM)
    const bool refm = h->refractory == lsm_lif::DENSE_REFM_REFRACTORY;
    const bool st = r.stateful();
    lsm_lif::dense_fn_t dfn = v.inmask      ? (v.incol ? lsm_lif::pick_dense_3(v.sl, v.wpc, refm, st)
                                                       : lsm_lif::pick_dense_2(v.sl, v.wpc, refm, st))
                              : lif_inreg(v) ? lsm_lif::pick_dense_1(v.sl, v.wpc, refm, st)
                                             : lsm_lif::pick_dense_0(v.sl, v.wpc, refm, st);
    LSM_REQUIRE(dfn != nullptr, "no dense kernel for SL=%d WPC=%d", v.sl, v.wpc);
    lsm_lif::DenseArgs a;
    set_common_args(&a, h, r);
    a.EinW = v.einw; a.ld = h->ld;
    a.wt = h->wt.get(); a.leak = v.leak.get(); a.oslot = v.oslot.get(); a.in_ent = v.in_ent.get();
    a.inmask = v.inmask.get();
    a.inperm = v.incol ? h->inperm.get() : nullptr;
    const size_t lds = dense_lds_bytes(h, v, r.n_steps);
    LSM_REQUIRE(lds <= 160 * 1024, "dense layout needs %zu bytes of LDS", lds);
    return launch(dfn, a, r, v.wpc, lds);
}

// The fused step launch (step_fused.hip, include/lsm_hip_step.h) runs the dense-row time loop behind the front end of the same
// clip: what run_dense would launch for a step inside the pipeline (waves_per_clip = -1, no spike matrix, trace, state or
// order), as its arguments.  The step kernel has the <SL, 4, 3, true> forms only: any other plan is LSM_ERR_UNSUPPORTED.
// `probe`: the shape alone is asked about (lsm_step_fused_supported), no buffer is looked at.
int lsm_lif::step_dense_args(const lsm_reservoir *h, int n_clips, int n_steps, const int32_t *key_ids, int n_keys,
                             float *features, int32_t *stats, bool probe, DenseArgs *out, int *sl_out, size_t *lds_out,
                             const StepState *state)
{
    LSM_REQUIRE(h != nullptr, "lsm_step_fused: null reservoir handle");
    LSM_REQUIRE(n_clips >= 1 && n_steps >= 1 && n_steps <= 65535, "bad n_clips/n_steps");
    RunArgs r;
    r.n_clips = n_clips; r.n_steps = n_steps; r.waves_per_clip = -1;
    if (!probe) {
        if (state) {
            // check_run's refusals of a segmented launch and of a continuation, in its order and words
            if (state->segmented) {
                LSM_REQUIRE(state->segment_steps >= 1, "segment_steps=%d must be >= 1", state->segment_steps);
                LSM_REQUIRE(n_steps % state->segment_steps == 0, "n_steps=%d is not a multiple of segment_steps=%d", n_steps,
                            state->segment_steps);
                LSM_REQUIRE(state->records != nullptr, "null records_out");
                LSM_REQUIRE((reinterpret_cast<uintptr_t>(state->records) & 15) == 0, "records_out must be 16-byte aligned");
                r.segmented = true; r.segment_steps = state->segment_steps; r.records = state->records;
            }
            LSM_REQUIRE(state->first_step >= 0, "first_step=%d must be >= 0", state->first_step);
            LSM_REQUIRE((long)state->first_step + n_steps <= 65535, "first_step + n_steps = %ld exceeds 65535 (the feature "
                        "records hold spike times in 16 bits)", (long)state->first_step + n_steps);
            LSM_REQUIRE(state->first_step == 0 || state->state_in != nullptr, "first_step=%d needs state_in (a run from reset "
                        "starts at 0)", state->first_step);
            LSM_REQUIRE((reinterpret_cast<uintptr_t>(state->state_in) & 15) == 0 &&
                        (reinterpret_cast<uintptr_t>(state->state_out) & 15) == 0, "state_in / state_out must be 16-byte aligned");
            LSM_REQUIRE(n_keys >= 0 && n_keys <= 8 && (n_keys == 0 || key_ids), "n_keys must be in [0, 8]");
            LSM_REQUIRE(n_keys == 0 || features, "null features_out with n_keys=%d", n_keys);
            r.from = true; r.state_in = state->state_in; r.state_out = state->state_out; r.first_step = state->first_step;
        } else {
            LSM_REQUIRE(n_keys >= 1 && n_keys <= 8 && key_ids, "n_keys must be in [1, 8]");
        }
        for (int k = 0; k < n_keys; ++k) LSM_REQUIRE(key_ids[k] >= 0 && key_ids[k] < 8, "key id %d out of range", key_ids[k]);
        LSM_REQUIRE(features != nullptr || state, "null features_out");
        int dev_now = -1;
        LSM_CHECK_HIP(hipGetDevice(&dev_now));
        LSM_REQUIRE(dev_now == h->device, "reservoir handle lives on device %d but the current device is %d", h->device,
                    dev_now);
        r.key_ids = key_ids; r.n_keys = n_keys; r.features = features; r.stats = stats;
    }
    RunPlan plan;
    if (const int rc = make_plan(h, n_clips, n_steps, r.waves_per_clip, &plan)) return rc;
    const Variant *v = plan.kernel == KERNEL_DENSE ? plan.v : nullptr;
    if (!v || v->wpc != 4 || !(v->sl == 1 || v->sl == 2 || v->sl == 4) || !v->inmask || !v->incol || h->C > 128 ||
        input_words(h) != 4 || h->refractory != lsm_lif::DENSE_REFM_REFRACTORY) {
        lsm_set_error("lsm_step_fused: the reservoir's launch for this shape is not the dense-row kernel with 4 waves per clip, "
                      "coloured input masks over 4 row words and the 2-step refractory masks");
        return LSM_ERR_UNSUPPORTED;
    }
    lsm_lif::DenseArgs a;
    set_common_args(&a, h, r);
    a.EinW = v->einw; a.ld = h->ld;
    a.wt = h->wt.get(); a.leak = v->leak.get(); a.oslot = v->oslot.get(); a.in_ent = v->in_ent.get();
    a.inmask = v->inmask.get();
    a.inperm = h->inperm.get();
    *out = a; *sl_out = v->sl; *lds_out = dense_lds_bytes(h, *v, n_steps);
    return LSM_OK;
}

static int run_sparse(const lsm_reservoir *h, const Variant &v, const RunArgs &r)
{
    lif_fn_t fn = pick_kernel(v.sl, v.wpc, lif_inreg(v), lif_seg_in_lds(h, v, r.n_steps), r.stateful());
    LSM_REQUIRE(fn != nullptr, "no kernel for SL=%d WPC=%d", v.sl, v.wpc);
    LifArgs a;
    set_common_args(&a, h, r);
    a.EinW = v.einw;
    a.rowptr = h->rowptr.get(); a.segoff = v.segoff.get();
    a.seg = v.seg.get(); a.syn = h->syn.get(); a.leak = v.leak.get(); a.oslot = v.oslot.get();
    a.in_ent = v.in_ent.get();
    return launch(fn, a, r, v.wpc, lif_lds_bytes(h, v, r.n_steps));
}

// Step 1 of a launch: what it refuses, in the order that decides which reason a caller with two bad arguments reads, and
// the plan (made before the workspace is looked at).  An empty batch is accepted before its buffers are.
static int check_run(const lsm_reservoir *h, const RunArgs &r, RunPlan *plan)
{
    LSM_REQUIRE(h != nullptr, "lsm_reservoir_run: null handle");
    LSM_REQUIRE(r.n_clips >= 0 && r.n_steps >= 1 && r.n_steps <= 65535, "bad n_clips/n_steps");
    if (r.segmented) {
        LSM_REQUIRE(r.segment_steps >= 1, "segment_steps=%d must be >= 1", r.segment_steps);
        LSM_REQUIRE(r.n_steps % r.segment_steps == 0, "n_steps=%d is not a multiple of segment_steps=%d", r.n_steps,
                    r.segment_steps);
        LSM_REQUIRE(r.records != nullptr || r.n_clips == 0, "null records_out");
        LSM_REQUIRE((reinterpret_cast<uintptr_t>(r.records) & 15) == 0, "records_out must be 16-byte aligned");
    }
    if (r.from) {
        LSM_REQUIRE(r.first_step >= 0, "first_step=%d must be >= 0", r.first_step);
        LSM_REQUIRE((long)r.first_step + r.n_steps <= 65535, "first_step + n_steps = %ld exceeds 65535 (the feature records hold "
                    "spike times in 16 bits)", (long)r.first_step + r.n_steps);
        LSM_REQUIRE(r.first_step == 0 || r.state_in != nullptr, "first_step=%d needs state_in (a run from reset starts at 0)",
                    r.first_step);
        LSM_REQUIRE((reinterpret_cast<uintptr_t>(r.state_in) & 15) == 0 && (reinterpret_cast<uintptr_t>(r.state_out) & 15) == 0,
                    "state_in / state_out must be 16-byte aligned");
        LSM_REQUIRE(r.n_keys >= 0 && r.n_keys <= 8 && (r.n_keys == 0 || r.key_ids), "n_keys must be in [0, 8]");
        LSM_REQUIRE(r.n_keys == 0 || r.features, "null features_out with n_keys=%d", r.n_keys);
    } else {
        LSM_REQUIRE(r.n_keys >= 1 && r.n_keys <= 8 && r.key_ids, "n_keys must be in [1, 8]");
    }
    LSM_REQUIRE((reinterpret_cast<uintptr_t>(r.clip_steps) & 3) == 0, "%s must be 4-byte aligned",
                r.streamed ? "clip_segments" : "clip_steps");
    LSM_REQUIRE(r.waves_per_clip >= -1 && r.waves_per_clip <= 16, "waves_per_clip must be -1 (pipelined), 0 (choose) or 1..16");
    if (r.n_clips == 0) return LSM_OK;          // empty batch: nothing to read or write
    LSM_REQUIRE(r.raster && (r.features || r.from), "null buffer");
    int dev_now = -1;
    LSM_CHECK_HIP(hipGetDevice(&dev_now));
    LSM_REQUIRE(dev_now == h->device, "reservoir handle lives on device %d but the current device is %d",
                h->device, dev_now);
    for (int k = 0; k < r.n_keys; ++k)
        LSM_REQUIRE(r.key_ids[k] >= 0 && r.key_ids[k] < 8, "key id %d out of range", r.key_ids[k]);
    const int prc = make_plan(h, r.n_clips, r.n_steps, r.waves_per_clip, plan);
    if (prc) return prc;
    if (r.workspace) {
        LSM_REQUIRE((reinterpret_cast<uintptr_t>(r.workspace) & 3) == 0, "workspace must be 4-byte aligned");
        LSM_REQUIRE(r.workspace_bytes >= lsm_reservoir_order_workspace(r.n_clips),
                    "workspace of %ld bytes, need %ld (lsm_reservoir_order_workspace)", r.workspace_bytes,
                    lsm_reservoir_order_workspace(r.n_clips));
    }
    return LSM_OK;
}

// Step 2: longest clips first, when the caller gave a workspace and the launch has more workgroups than the chip has CUs
// (else every clip starts at once).
static int order_clips(const lsm_reservoir *h, RunArgs *r)
{
    if (!r->workspace || h->cus <= 0 || r->n_clips <= h->cus) return LSM_OK;
    int32_t *keys = static_cast<int32_t *>(r->workspace);
    int32_t *ord = keys + r->n_clips;
    if (r->clip_steps)      // the bytes inside every clip's own length
        hipLaunchKernelGGL(clip_keys_ragged_kernel, dim3(r->n_clips), dim3(256), 0, (hipStream_t)r->stream, r->raster,
                           h->C, r->n_steps, r->clip_steps, r->n_clips, keys, r->streamed ? r->segment_steps : 0);
    else
        hipLaunchKernelGGL(clip_keys_kernel, dim3(r->n_clips), dim3(256), 0, (hipStream_t)r->stream, r->raster,
                           (long)h->C * r->n_steps, r->n_clips, keys);
    hipLaunchKernelGGL(clip_rank_kernel, dim3((r->n_clips + 255) / 256), dim3(256), 0, (hipStream_t)r->stream,
                       keys, r->n_clips, ord);
    LSM_CHECK_HIP(hipGetLastError());
    r->order = ord;
    return LSM_OK;
}

// Step 3: the planned kernel.
static int dispatch(const lsm_reservoir *h, const RunPlan &plan, const RunArgs &r)
{
    if (plan.pv) return run_pairs(h, *plan.pv, r);
    if (plan.rv) return run_quads(h, *plan.rv, r);
    return plan.kernel == KERNEL_DENSE ? run_dense(h, *plan.v, r) : run_sparse(h, *plan.v, r);
}

// Every run export ends here with the request it filled.
static int reservoir_run(const lsm_reservoir *h, RunArgs *r)
{
    RunPlan plan;
    int rc = check_run(h, *r, &plan);
    if (rc != LSM_OK || r->n_clips == 0) return rc;    // refused, or an empty batch: accepted, but no plan was made for it
    rc = order_clips(h, r);
    return rc != LSM_OK ? rc : dispatch(h, plan, *r);
}

// What all six run exports are given: the clips, the outputs of every step, the layout request and the stream.
static RunArgs run_args(const uint8_t *spikes_u8, int n_clips, int n_steps, uint8_t *spike_matrix_out, float *v_trace_out,
                        int32_t *stats_out, int waves_per_clip, void *stream)
{
    RunArgs r;
    r.raster = spikes_u8; r.n_clips = n_clips; r.n_steps = n_steps;
    r.spike_matrix = spike_matrix_out; r.v_trace = v_trace_out; r.stats = stats_out;
    r.waves_per_clip = waves_per_clip; r.stream = stream;
    return r;
}

extern "C" __attribute__((visibility("default")))
int lsm_reservoir_run(const lsm_reservoir *h, const uint8_t *spikes_u8, int n_clips, int n_steps,
                      const int32_t *key_ids, int n_keys, float *features_out,
                      uint8_t *spike_matrix_out, float *v_trace_out, int32_t *stats_out,
                      int waves_per_clip, void *stream)
{
    RunArgs r = run_args(spikes_u8, n_clips, n_steps, spike_matrix_out, v_trace_out, stats_out, waves_per_clip, stream);
    r.key_ids = key_ids; r.n_keys = n_keys; r.features = features_out;
    return reservoir_run(h, &r);
}

extern "C" __attribute__((visibility("default")))
int lsm_reservoir_run_ordered(const lsm_reservoir *h, const uint8_t *spikes_u8, int n_clips, int n_steps,
                              const int32_t *key_ids, int n_keys, float *features_out,
                              uint8_t *spike_matrix_out, float *v_trace_out, int32_t *stats_out,
                              int waves_per_clip, void *workspace, long workspace_bytes, void *stream)
{
    LSM_REQUIRE(workspace != nullptr || n_clips == 0, "lsm_reservoir_run_ordered: null workspace");
    RunArgs r = run_args(spikes_u8, n_clips, n_steps, spike_matrix_out, v_trace_out, stats_out, waves_per_clip, stream);
    r.key_ids = key_ids; r.n_keys = n_keys; r.features = features_out;
    r.workspace = workspace; r.workspace_bytes = workspace_bytes;
    return reservoir_run(h, &r);
}

extern "C" __attribute__((visibility("default")))
long lsm_reservoir_state_bytes(const lsm_reservoir *h)
{
    return h ? lsm_lif::state_bytes(h->N, h->n_out) : (long)LSM_ERR_ARG;
}

// lsm_reservoir_run / _run_ordered from a saved state and into one: the same plan, the same tables, the ST forms of the
// kernels (lif_common.h).  With neither state it is lsm_reservoir_run.
extern "C" __attribute__((visibility("default")))
int lsm_reservoir_run_from(const lsm_reservoir *h, const uint8_t *spikes_u8, int n_clips, int n_steps,
                           int first_step, const void *state_in, void *state_out,
                           const int32_t *key_ids, int n_keys, float *features_out,
                           uint8_t *spike_matrix_out, float *v_trace_out, int32_t *stats_out,
                           int waves_per_clip, void *order_workspace, long order_workspace_bytes, void *stream)
{
    RunArgs r = run_args(spikes_u8, n_clips, n_steps, spike_matrix_out, v_trace_out, stats_out, waves_per_clip, stream);
    r.key_ids = key_ids; r.n_keys = n_keys; r.features = features_out;
    r.workspace = order_workspace; r.workspace_bytes = order_workspace_bytes;
    r.from = true; r.state_in = state_in; r.state_out = state_out; r.first_step = first_step;
    return reservoir_run(h, &r);
}

// lsm_reservoir_run_from with the feature bookkeeping cut every segment_steps steps (SPEC.md §4b): always the ST forms,
// which close each output neuron's record into records_out at the segment ends (lif_common.h, segment_close).
extern "C" __attribute__((visibility("default")))
int lsm_reservoir_run_segments(const lsm_reservoir *h, const uint8_t *spikes_u8, int n_clips, int n_steps,
                               int segment_steps, int first_step, const void *state_in, void *state_out, void *records_out,
                               const int32_t *key_ids, int n_keys, float *features_out,
                               uint8_t *spike_matrix_out, float *v_trace_out, int32_t *stats_out,
                               int waves_per_clip, void *order_workspace, long order_workspace_bytes, void *stream)
{
    RunArgs r = run_args(spikes_u8, n_clips, n_steps, spike_matrix_out, v_trace_out, stats_out, waves_per_clip, stream);
    r.key_ids = key_ids; r.n_keys = n_keys; r.features = features_out;
    r.workspace = order_workspace; r.workspace_bytes = order_workspace_bytes;
    r.from = true; r.state_in = state_in; r.state_out = state_out; r.first_step = first_step;
    r.segmented = true; r.segment_steps = segment_steps; r.records = records_out;
    return reservoir_run(h, &r);
}

// lsm_reservoir_run_from whose clips run clip_steps[b] (clamped into [0, n_steps]) steps each (SPEC.md §4c): the same
// refusals, the plan and the LDS image of n_steps, always the ST forms; the kernels read the count once per workgroup.
extern "C" __attribute__((visibility("default")))
int lsm_reservoir_run_ragged(const lsm_reservoir *h, const uint8_t *spikes_u8, int n_clips, int n_steps,
                             const int32_t *clip_steps, int first_step, const void *state_in, void *state_out,
                             const int32_t *key_ids, int n_keys, float *features_out,
                             uint8_t *spike_matrix_out, float *v_trace_out, int32_t *stats_out,
                             int waves_per_clip, void *order_workspace, long order_workspace_bytes, void *stream)
{
    RunArgs r = run_args(spikes_u8, n_clips, n_steps, spike_matrix_out, v_trace_out, stats_out, waves_per_clip, stream);
    r.key_ids = key_ids; r.n_keys = n_keys; r.features = features_out;
    r.workspace = order_workspace; r.workspace_bytes = order_workspace_bytes;
    r.from = true; r.state_in = state_in; r.state_out = state_out; r.first_step = first_step;
    r.ragged = true; r.clip_steps = clip_steps;
    return reservoir_run(h, &r);
}

// One thread per (clip, window, output neuron): §4a's merge folded over the window's records, then the neuron's n_keys
// features (key-major rows, as write_features writes them).
struct SegmentFeatureArgs {
    const uint4 *rec;          // (B, G, n_out)
    float *features;           // (B, W, n_keys * n_out)
    int B, G, S, K, H, W, n_out, n_keys, burst_isi_max;
    int key_ids[8];
    const int32_t *valid;      // lsm_segment_features_ragged (SPEC.md §4d): (B) valid segments of every clip, clamped into [0, G]
};

// The row of window wdw of clip b for output neuron o (bw = b * W + wdw): both kernels below.
__device__ __forceinline__ void segment_window_row(const SegmentFeatureArgs &a, int b, int wdw, long bw, int o)
{
    const uint4 *rec = a.rec + ((size_t)b * a.G + (size_t)wdw * a.H) * a.n_out + o;
    uint4 f = make_uint4(0, 0, 0, 0);
    for (int j = 0; j < a.K; ++j)
        f = lsm_lif::merge_feature_records(f, rec[(size_t)j * a.n_out], (uint32_t)(j * a.S), a.burst_isi_max);
    const int n = (int)(f.x & 0xFFFFu), bursts = (int)(f.x >> 16);
    const int first = (int)(f.y & 0xFFFFu), last = (int)(f.y >> 16);
    float *row = a.features + (size_t)bw * a.n_keys * a.n_out + o;
    for (int k = 0; k < a.n_keys; ++k)
        row[(size_t)k * a.n_out] = lsm_lif::feature_value(a.key_ids[k], n, bursts, first, last, f.z, f.w, a.K * a.S);
}

__global__ __launch_bounds__(256) void segment_features_kernel(const SegmentFeatureArgs a)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)a.B * a.W * a.n_out;
    if (idx >= total) return;
    const int o = (int)(idx % a.n_out);
    const long bw = idx / a.n_out;
    segment_window_row(a, (int)(bw / a.W), (int)(bw % a.W), bw, o);
}

// The same over records of which clip b has Gv_b = clamp(valid[b], 0, G) (SPEC.md §4d): a thread whose window is not
// complete -- wdw * H + K > Gv_b -- returns without storing, so rows at w >= W_b keep what they held.
__global__ __launch_bounds__(256) void segment_features_ragged_kernel(const SegmentFeatureArgs a)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)a.B * a.W * a.n_out;
    if (idx >= total) return;
    const int o = (int)(idx % a.n_out);
    const long bw = idx / a.n_out;
    const int wdw = (int)(bw % a.W);
    const int b = (int)(bw / a.W);
    const int gv = min(max(a.valid[b], 0), a.G);
    if ((long)wdw * a.H + a.K > gv) return;
    segment_window_row(a, b, wdw, bw, o);
}

enum SegmentCounts { ALL_SEGMENTS, CLIP_SEGMENTS };     // every clip has all n_segments records / clip_segments[b] of them

static int segment_features(const lsm_reservoir *h, const void *records, int n_clips, int n_segments, int segment_steps,
                            int window_segments, int hop_segments, const int32_t *key_ids, int n_keys, float *features_out,
                            void *stream, SegmentCounts counts, const int32_t *clip_segments)
{
    LSM_REQUIRE(h != nullptr, "lsm_segment_features: null handle");
    LSM_REQUIRE(n_clips >= 0 && n_segments >= 1, "bad n_clips/n_segments");
    LSM_REQUIRE(segment_steps >= 1, "segment_steps=%d must be >= 1", segment_steps);
    LSM_REQUIRE(window_segments >= 1 && window_segments <= n_segments, "window_segments=%d must be in [1, n_segments=%d]",
                window_segments, n_segments);
    LSM_REQUIRE(hop_segments >= 1, "hop_segments=%d must be >= 1", hop_segments);
    LSM_REQUIRE((long)window_segments * segment_steps <= 65535, "a window of %d segments of %d steps exceeds 65535 steps "
                "(the feature records hold spike times in 16 bits)", window_segments, segment_steps);
    LSM_REQUIRE(n_keys >= 1 && n_keys <= 8 && key_ids, "n_keys must be in [1, 8]");
    for (int k = 0; k < n_keys; ++k)
        LSM_REQUIRE(key_ids[k] >= 0 && key_ids[k] < 8, "key id %d out of range", key_ids[k]);
    LSM_REQUIRE((reinterpret_cast<uintptr_t>(records) & 15) == 0, "records must be 16-byte aligned");
    LSM_REQUIRE((reinterpret_cast<uintptr_t>(clip_segments) & 3) == 0, "clip_segments must be 4-byte aligned");
    if (n_clips == 0) return LSM_OK;
    LSM_REQUIRE(records && features_out, "null buffer");
    LSM_REQUIRE(counts == ALL_SEGMENTS || clip_segments, "null clip_segments");
    int dev_now = -1;
    LSM_CHECK_HIP(hipGetDevice(&dev_now));
    LSM_REQUIRE(dev_now == h->device, "reservoir handle lives on device %d but the current device is %d",
                h->device, dev_now);
    SegmentFeatureArgs a;
    a.rec = static_cast<const uint4 *>(records); a.features = features_out;
    a.B = n_clips; a.G = n_segments; a.S = segment_steps; a.K = window_segments; a.H = hop_segments;
    a.W = (n_segments - window_segments) / hop_segments + 1;
    a.n_out = h->n_out; a.n_keys = n_keys; a.burst_isi_max = h->burst_isi_max;
    for (int k = 0; k < 8; ++k) a.key_ids[k] = k < n_keys ? key_ids[k] : 0;
    a.valid = clip_segments;
    const long total = (long)a.B * a.W * a.n_out;
    LSM_REQUIRE((total + 255) / 256 <= 0x7FFFFFFFL, "too many (clip, window, output neuron) triples: %ld", total);
    if (total == 0) return LSM_OK;
    hipLaunchKernelGGL(counts == CLIP_SEGMENTS ? segment_features_ragged_kernel : segment_features_kernel,
                       dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}

extern "C" __attribute__((visibility("default")))
int lsm_segment_features(const lsm_reservoir *h, const void *records, int n_clips, int n_segments, int segment_steps,
                         int window_segments, int hop_segments, const int32_t *key_ids, int n_keys, float *features_out,
                         void *stream)
{
    return segment_features(h, records, n_clips, n_segments, segment_steps, window_segments, hop_segments, key_ids, n_keys,
                            features_out, stream, ALL_SEGMENTS, nullptr);
}

// ---- streams (SPEC.md §4d, include/lsm_hip_streams.h) --------------------------------------------------------------------
// lsm_reservoir_run_segments whose clips run clip_segments[b] whole segments each and which keeps no cumulative record: no
// first_step (nothing in the launch depends on a clip's position on its own timeline), no features, the feat block of
// state_in is not read and that of state_out is written as zeros.  Always the ST forms.
extern "C" __attribute__((visibility("default")))
int lsm_reservoir_run_stream(const lsm_reservoir *h, const uint8_t *spikes_u8, int n_clips, int n_steps,
                             int segment_steps, const int32_t *clip_segments, const void *state_in, void *state_out,
                             void *records_out, uint8_t *spike_matrix_out, float *v_trace_out, int32_t *stats_out,
                             int waves_per_clip, void *order_workspace, long order_workspace_bytes, void *stream)
{
    RunArgs r = run_args(spikes_u8, n_clips, n_steps, spike_matrix_out, v_trace_out, stats_out, waves_per_clip, stream);
    r.workspace = order_workspace; r.workspace_bytes = order_workspace_bytes;
    r.from = true; r.state_in = state_in; r.state_out = state_out;
    r.segmented = true; r.segment_steps = segment_steps; r.records = records_out;
    r.ragged = true; r.clip_steps = clip_segments; r.streamed = true;
    return reservoir_run(h, &r);
}

// lsm_segment_features over records of which every clip has a valid count of its own.
extern "C" __attribute__((visibility("default")))
int lsm_segment_features_ragged(const lsm_reservoir *h, const void *records, int n_clips, int n_segments,
                                const int32_t *clip_segments, int segment_steps, int window_segments, int hop_segments,
                                const int32_t *key_ids, int n_keys, float *features_out, void *stream)
{
    return segment_features(h, records, n_clips, n_segments, segment_steps, window_segments, hop_segments, key_ids, n_keys,
                            features_out, stream, CLIP_SEGMENTS, clip_segments);
}

// The plan for lsm_reservoir_plan and _row_request_bytes, behind the two refusals they share.
static int plan_request(const lsm_reservoir *h, int n_clips, int n_steps, int waves_per_clip, RunPlan *p)
{
    LSM_REQUIRE(n_clips >= 0 && n_steps >= 1 && n_steps <= 65535, "bad n_clips/n_steps");
    LSM_REQUIRE(waves_per_clip >= -1 && waves_per_clip <= 16, "waves_per_clip must be -1 (pipelined), 0 (choose) or 1..16");
    return make_plan(h, n_clips, n_steps, waves_per_clip, p);
}

// Largest n_steps make_plan accepts for this batch and waves_per_clip: every layout's LDS image grows with the steps, so
// the accepted lengths are 1 .. that.
extern "C" __attribute__((visibility("default")))
int lsm_reservoir_max_steps(const lsm_reservoir *h, int n_clips, int waves_per_clip)
{
    LSM_REQUIRE(h != nullptr, "lsm_reservoir_max_steps: null handle");
    LSM_REQUIRE(n_clips >= 0, "bad n_clips");
    LSM_REQUIRE(waves_per_clip >= -1 && waves_per_clip <= 16, "waves_per_clip must be -1 (pipelined), 0 (choose) or 1..16");
    RunPlan p;
    const int rc = make_plan(h, n_clips, 1, waves_per_clip, &p);
    if (rc) return rc;                           // not even one step: the plan's own error
    int lo = 1, hi = 65535;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        RunPlan q;
        if (make_plan(h, n_clips, mid, waves_per_clip, &q) == LSM_OK) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Introspection for tests and the bench, read off a made plan: the layout chosen for a batch (waves per clip, neuron slots
// per lane), LDS bytes per workgroup, bytes of the weight table the kernel gathers its rows from and the mean bytes one row
// request moves, the kernel's input form (lsm_reservoir_input_mode) and which ring-row form it is: 0 not ring rows, 1 quads
// with contiguous ownership, 2 strided quads (lif_ring.h), 3 pair blocks (lif_pair.h).
struct PlanFacts {
    int wpc, slots, input_mode, ring_form;
    size_t lds_bytes, table_bytes;
    double row_request_bytes;
};

static PlanFacts plan_facts(const lsm_reservoir *h, const RunPlan &p, int n_steps)
{
    const double n = (double)h->N;
    PlanFacts f;
    if (p.pv) {
        const PairVariant &v = *p.pv;
        f.wpc = v.wpc; f.slots = v.bl * 2;
        f.lds_bytes = pair_lds_bytes(h, v, n_steps);
        // ring windows + this layout's lists + its row records
        f.table_bytes = (size_t)h->N * h->band_pitch + v.n_rem * 8 + (size_t)h->N * v.wpc * 16;
        f.row_request_bytes = (h->band_bytes_sum + (double)v.n_rem * 8.0) / n + v.wpc * 16.0;
        f.input_mode = v.inform == 3 ? 11 : (v.inform == 2 ? 15 : 14);
        f.ring_form = 3;
    } else if (p.rv) {
        const RingVariant &v = *p.rv;
        f.wpc = v.wpc; f.slots = v.ql * 4;
        f.lds_bytes = ring_lds_bytes(h, v, n_steps);
        // ring windows + this layout's lists of the synapses outside them + their row pointers
        f.table_bytes = (size_t)h->N * h->band_pitch + v.n_rem * 8 + ((size_t)h->N * v.wpc + 1) * 4;
        f.row_request_bytes = (h->band_bytes_sum + (double)v.n_rem * 8.0) / n + (v.wpc + 1) * 4.0;
        f.input_mode = v.inmask ? (v.incol ? 13 : 12) : (ring_inreg(v) ? 11 : 10);
        f.ring_form = v.strided ? 2 : 1;
    } else {
        const Variant &v = *p.v;
        const bool dense = p.kernel == KERNEL_DENSE;
        f.wpc = v.wpc; f.slots = v.sl;
        f.lds_bytes = dense ? dense_lds_bytes(h, v, n_steps) : lif_lds_bytes(h, v, n_steps);
        f.table_bytes = dense ? (size_t)h->N * h->ld * 4 : h->nnz * 8 + ((size_t)h->N + 1) * 4;
        f.row_request_bytes = dense ? (double)h->ld * 4.0 : (double)h->nnz * 8.0 / n + 8.0;
        f.input_mode = !dense ? 20 : v.inmask ? (v.incol ? 3 : 2) : (lif_inreg(v) ? 1 : 0);
        f.ring_form = 0;
    }
    return f;
}

extern "C" __attribute__((visibility("default")))
int lsm_reservoir_plan(const lsm_reservoir *h, int n_clips, int n_steps, int waves_per_clip, int *kernel_out,
                       int *wpc_out, int *slots_out, int *lds_bytes_out, long *table_bytes_out)
{
    LSM_REQUIRE(h != nullptr, "lsm_reservoir_plan: null handle");
    RunPlan p;
    const int rc = plan_request(h, n_clips, n_steps, waves_per_clip, &p);
    if (rc) return rc;
    const PlanFacts f = plan_facts(h, p, n_steps);
    if (kernel_out) *kernel_out = p.kernel;
    if (wpc_out) *wpc_out = f.wpc;
    if (slots_out) *slots_out = f.slots;
    if (lds_bytes_out) *lds_bytes_out = (int)f.lds_bytes;
    if (table_bytes_out) *table_bytes_out = (long)f.table_bytes;
    return LSM_OK;
}

extern "C" __attribute__((visibility("default")))
int lsm_reservoir_layout(const lsm_reservoir *h, int n_clips, int n_steps, int waves_per_clip,
                         int *wpc_out, int *slots_out, int *lds_bytes_out)
{
    return lsm_reservoir_plan(h, n_clips, n_steps, waves_per_clip, nullptr, wpc_out, slots_out, lds_bytes_out, nullptr);
}

extern "C" __attribute__((visibility("default")))
int lsm_reservoir_row_request_bytes(const lsm_reservoir *h, int n_clips, int n_steps, int waves_per_clip,
                                    double *mean_bytes_out)
{
    LSM_REQUIRE(h != nullptr && mean_bytes_out != nullptr, "lsm_reservoir_row_request_bytes: null argument");
    RunPlan p;
    const int rc = plan_request(h, n_clips, n_steps, waves_per_clip, &p);
    if (rc) return rc;
    *mean_bytes_out = plan_facts(h, p, n_steps).row_request_bytes;
    return LSM_OK;
}

// The plan for lsm_reservoir_input_mode and _ring_form, which refuse only a null handle and leave no message.
static int quiet_plan(const lsm_reservoir *h, int n_clips, int n_steps, int waves_per_clip, RunPlan *p)
{
    if (h == nullptr) return LSM_ERR_ARG;
    return make_plan(h, n_clips, n_steps, waves_per_clip, p) == LSM_OK ? LSM_OK : LSM_ERR_UNSUPPORTED;
}

extern "C" __attribute__((visibility("default")))
int lsm_reservoir_input_mode(const lsm_reservoir *h, int n_clips, int n_steps, int waves_per_clip)
{
    RunPlan p;
    const int rc = quiet_plan(h, n_clips, n_steps, waves_per_clip, &p);
    return rc ? rc : plan_facts(h, p, n_steps).input_mode;
}

extern "C" __attribute__((visibility("default")))
int lsm_reservoir_ring_form(const lsm_reservoir *h, int n_clips, int n_steps, int waves_per_clip)
{
    RunPlan p;
    const int rc = quiet_plan(h, n_clips, n_steps, waves_per_clip, &p);
    return rc ? rc : plan_facts(h, p, n_steps).ring_form;
}

// Which kernel lsm_reservoir_run would launch for this handle: 1 sparse, 2 dense rows, 3 ring rows -- for the
// reference's 400 time steps and waves_per_clip = 0 (lsm_reservoir_plan answers for any launch).
extern "C" __attribute__((visibility("default")))
int lsm_reservoir_kernel_in_use(const lsm_reservoir *h)
{
    if (h == nullptr) return LSM_ERR_ARG;
    RunPlan p;
    if (make_plan(h, 1, 400, 0, &p) != LSM_OK) return want_ring(h) ? KERNEL_RING : (use_dense(h) ? KERNEL_DENSE : KERNEL_SPARSE);
    return p.kernel;
}
