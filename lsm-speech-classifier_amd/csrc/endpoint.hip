// Stream endpointing for gfx950 (SPEC.md §1.17, include/lsm_hip_endpoint.h): per stream and push, the energies of the new
// 160-sample bins, their activity against a sliding maximum, the utterances the state machine closes, and those utterances'
// samples moved into the slots of a ragged batch.
//
// Layout.  One workgroup of 256 threads (four wave64) per stream, five phases with LDS between them.
//   history    the block's integers (endpoint_body.h: clamped on the way in) and its last W - 1 values e^ into LDS, in front of
//              the places of this push's bins, so that the window of bin n is LDS words n .. n + W - 1 whatever n is.
//   energies   bin_energy.h, the trimmer's code: tiles of up to 64 bins staged with coalesced loads, one lane per row.
//   activity   a thread per bin walks its window of e^ for the maximum (max is exact and order-free), then the two compares.
//   machine    one lane runs the bins of the push in order (endpoint_body.h) and leaves a copy record (first bin, bins, flags)
//              per kept utterance in LDS: at most 4096 bins of a few integer operations.
//   copy       all lanes: the counts, then every kept utterance from the audio ring (bins before this push) and the push's
//              row into its slot and +0.0 behind it, by 16-byte accesses where the launch's pointers allow and by words
//              otherwise; a barrier; then the new block -- integers, e^ ring, audio ring -- or zeros for a finished stream.
//              Samples move as words, so -0.0 and NaN payloads stay.  The ring is read before the barrier and written
//              behind it: state_out may be state_in.
// Every index is formed from clamped values: 0 <= h_b <= n_hops, -M < first bin of an utterance, its last bin < h_b, at most
// M bins, slot < max_utts; ring slots are residues mod M and mod W - 1.
// state_in and state_out follow DESIGN.md "The state block"; the block is whole 16-byte pieces and an idle stream's travels as such.
#include "lsm_common.h"
#include "bin_energy.h"
#include "endpoint_body.h"
#include "stream_state.h"
#include <cmath>

namespace {

using namespace lsm_endpoint;
using lsm_energy::PITCH;

constexpr int THREADS = 256;

struct EndpointArgs {
    const float *audio;                     // (n_streams, n_hops * 160)
    const int32_t *stream_hops, *finish;    // (n_streams) or null
    const unsigned char *state_in;          // (n_streams, state_bytes) or null
    unsigned char *state_out;               // the same or null
    float *utt_audio;                       // (n_streams, max_utts, 160 * M)
    int32_t *utt_bins;                      // (n_streams, max_utts)
    int64_t *utt_first;                     // (n_streams, max_utts) or null
    int32_t *utt_flags, *utt_count;         // (n_streams, max_utts), (n_streams) or null
    double *energy_out;                     // (n_streams, n_hops) or null
    unsigned char *active_out;              // (n_streams, n_hops) or null
    double ratio, floor;
    long state_bytes;
    int n_hops, W, P, G, A, M, max_utts, tile_bins, records;
};

// Dynamic LDS: W - 1 + n_hops float64 (history and this push's e^), the energy tile, the copy records, the activity bytes
__host__ __device__ inline int tile_bins_of(int n_hops)
{
    return n_hops < lsm_energy::TILE_BINS ? n_hops : lsm_energy::TILE_BINS;
}

__host__ __device__ inline int records_of(int n_hops, int max_utts)
{
    return max_utts < n_hops + 1 ? max_utts : n_hops + 1;      // a bin closes one utterance at most, the finish one more
}

inline size_t lds_bytes(int n_hops, int W, int max_utts)
{
    return 8u * (size_t)(W - 1 + n_hops) + 4u * (size_t)(tile_bins_of(n_hops) * PITCH + (tile_bins_of(n_hops) * PITCH & 1))
           + 12u * (size_t)records_of(n_hops, max_utts) + (size_t)((n_hops + 15) / 16 * 16);
}

__device__ inline void copy_words(uint32_t *dst, const uint32_t *src, int n, bool quads, int tid)
{
    if (quads) {
        for (int q = tid; q < n / 4; q += THREADS) reinterpret_cast<uint4 *>(dst)[q] = reinterpret_cast<const uint4 *>(src)[q];
    } else {
        for (int m = tid; m < n; m += THREADS) dst[m] = src[m];
    }
}

__device__ inline void zero_words(uint32_t *dst, int n, bool quads, int tid)
{
    if (quads) {
        for (int q = tid; q < n / 4; q += THREADS) reinterpret_cast<uint4 *>(dst)[q] = make_uint4(0u, 0u, 0u, 0u);
    } else {
        for (int m = tid; m < n; m += THREADS) dst[m] = 0u;
    }
}

__global__ __launch_bounds__(THREADS) void endpoint_kernel(const EndpointArgs a)
{
    extern __shared__ double ehat[];                                // history, then this push's bins
    const int Wr = a.W - 1;
    float *tile = reinterpret_cast<float *>(ehat + Wr + a.n_hops);
    const int tile_words = a.tile_bins * PITCH + (a.tile_bins * PITCH & 1);
    int *rec = reinterpret_cast<int *>(tile + tile_words);          // (s, bins, flags) per kept utterance
    unsigned char *act = reinterpret_cast<unsigned char *>(rec + 3 * a.records);
    __shared__ Header s_in, s_out;
    __shared__ int s_count;

    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int M = a.M;
    const int h = clamp_hops(a.stream_hops ? a.stream_hops[b] : a.n_hops, a.n_hops);
    const bool fin = a.finish && a.finish[b] != 0;
    const lsm_state::StateBlock blk = lsm_state::state_block(a.state_in, a.state_out, b, (size_t)a.state_bytes);
    const unsigned char *st_in = blk.sin;
    unsigned char *st_out = blk.sout;
    int32_t *bins_out = a.utt_bins + b * (size_t)a.max_utts;

    // ---- a stream that delivers nothing and does not end: no utterance, the block as it is -----------------------------------
    if (h == 0 && !fin) {
        for (int u = tid; u < a.max_utts; u += THREADS) bins_out[u] = 0;
        if (tid == 0 && a.utt_count) a.utt_count[b] = 0;
        if (blk.copy) {               // DESIGN.md "The state block"; the block is whole 16-byte pieces
            const int quads = (int)(a.state_bytes / 16);
            for (int q = tid; q < quads; q += THREADS)
                reinterpret_cast<uint4 *>(st_out)[q] = st_in ? reinterpret_cast<const uint4 *>(st_in)[q] : make_uint4(0u, 0u, 0u, 0u);
        }
        return;
    }

    // ---- history -------------------------------------------------------------------------------------------------------------
    if (tid < (int)(sizeof(Header) / 4))
        reinterpret_cast<uint32_t *>(&s_in)[tid] = st_in ? reinterpret_cast<const uint32_t *>(st_in)[tid] : 0u;
    __syncthreads();
    const int64_t n0 = first_bin(s_in);
    const long ring_e = energy_ring_bytes(a.W);
    {
        const double *e_ring = st_in ? reinterpret_cast<const double *>(st_in + sizeof(Header)) : nullptr;
        const int base = Wr ? (int)(n0 % Wr) : 0;
        for (int k = tid; k < Wr; k += THREADS) {                   // bin n0 - Wr + k
            double v = 0.0;
            if (e_ring && n0 - Wr + k >= 0) {
                v = e_ring[(base + k) % Wr];                        // (n0 - Wr + k) mod Wr
                if (!(v >= 0.0 && std::isfinite(v))) v = 0.0;       // what this code never stored: a block from elsewhere
            }
            ehat[k] = v;
        }
    }

    // ---- energies ------------------------------------------------------------------------------------------------------------
    const float *in = a.audio + b * (size_t)a.n_hops * HOP;
    double *e_out = a.energy_out ? a.energy_out + b * (size_t)a.n_hops : nullptr;
    for (int j0 = 0; j0 < h; j0 += a.tile_bins) {
        const int nbt = min(a.tile_bins, h - j0);
        lsm_energy::stage_bins<THREADS>(in, HOP * h, j0, nbt, tile, tid);       // < 160 * h <= 160 * n_hops
        __syncthreads();
        if (tid < nbt) {
            const double e = lsm_energy::row_energy(tile + tid * PITCH);
            if (e_out) e_out[j0 + tid] = e;
            ehat[Wr + j0 + tid] = std::isfinite(e) ? e : 0.0;
        }
        __syncthreads();
    }
    if (h == 0) __syncthreads();                                    // the history, where no tile ran

    // ---- activity ------------------------------------------------------------------------------------------------------------
    // bin j's window is ehat[j .. j + Wr]; bins before the stream's start hold +0.0, which no maximum of values >= 0 notices
    for (int j = tid; j < h; j += THREADS) {
        const double e = ehat[Wr + j];
        double most = e;
        for (int i = 0; i < Wr; ++i) most = fmax(most, ehat[j + i]);
        const bool on = e > most * a.ratio && e > a.floor;
        act[j] = on ? 1 : 0;
        if (a.active_out) a.active_out[b * (size_t)a.n_hops + j] = on ? 1 : 0;
    }
    __syncthreads();

    // ---- machine -------------------------------------------------------------------------------------------------------------
    if (tid == 0) {
        Machine m = load(s_in, a.G, M);
        int count = 0;
        Closed c;
        for (int j = 0; j < h; ++j) {
            if (step(m, j, act[j] != 0, a.P, a.G, a.A, M, c) && c.kept && count < a.records) {
                rec[3 * count] = c.s;
                rec[3 * count + 1] = c.bins;
                rec[3 * count + 2] = c.flags;
                ++count;
            }
        }
        if (fin && finish(m, h, a.P, a.A, c) && c.kept && count < a.records) {
            rec[3 * count] = c.s;
            rec[3 * count + 1] = c.bins;
            rec[3 * count + 2] = c.flags;
            ++count;
        }
        s_count = count;
        store(m, n0, h, s_out);
    }
    __syncthreads();

    // ---- copy ----------------------------------------------------------------------------------------------------------------
    const int count = s_count;                                      // <= records <= max_utts
    for (int u = tid; u < a.max_utts; u += THREADS) {
        const bool live = u < count;
        bins_out[u] = live ? rec[3 * u + 1] : 0;
        if (live && a.utt_first) a.utt_first[b * (size_t)a.max_utts + u] = n0 + rec[3 * u];
        if (live && a.utt_flags) a.utt_flags[b * (size_t)a.max_utts + u] = rec[3 * u + 2];
    }
    if (tid == 0 && a.utt_count) a.utt_count[b] = count;

    const int ring_base = (int)(n0 % M);
    const uint32_t *ring_in = st_in ? reinterpret_cast<const uint32_t *>(st_in + sizeof(Header) + ring_e) : nullptr;
    const uint32_t *push = reinterpret_cast<const uint32_t *>(in);
    // the state blocks and the slot pitch are multiples of 16 bytes: the two base pointers decide for the whole launch
    const bool quads = ((reinterpret_cast<uintptr_t>(a.audio) | reinterpret_cast<uintptr_t>(a.utt_audio)) & 15u) == 0;
    const int row_words = HOP * M;
    for (int u = 0; u < count; ++u) {
        const int s = max(rec[3 * u], -(M - 1));                    // the machine's own bounds, held again where they address
        const int nb = min(rec[3 * u + 1], min(M, h - s));
        uint32_t *row = reinterpret_cast<uint32_t *>(a.utt_audio) + (b * (size_t)a.max_utts + u) * (size_t)row_words;
        for (int k = 0; k < nb; ++k) {
            const int r = s + k;                                    // -M < r < h
            if (r >= 0) {                                           // the push's bins lie side by side: one copy for the rest
                copy_words(row + HOP * k, push + HOP * r, HOP * (nb - k), quads, tid);
                break;
            }
            const int slot = (ring_base + r + M) % M;
            if (ring_in) copy_words(row + HOP * k, ring_in + HOP * slot, HOP, quads, tid);
            else zero_words(row + HOP * k, HOP, quads, tid);
        }
        zero_words(row + HOP * max(nb, 0), row_words - HOP * max(nb, 0), quads, tid);
    }
    __syncthreads();                                                // every read of state_in lies in front of this barrier

    // ---- the new block -------------------------------------------------------------------------------------------------------
    if (!st_out) return;
    if (fin) {
        const int n_quads = (int)(a.state_bytes / 16);
        for (int q = tid; q < n_quads; q += THREADS) reinterpret_cast<uint4 *>(st_out)[q] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    if (tid < (int)(sizeof(Header) / 4)) reinterpret_cast<uint32_t *>(st_out)[tid] = reinterpret_cast<const uint32_t *>(&s_out)[tid];
    {
        double *e_ring = reinterpret_cast<double *>(st_out + sizeof(Header));
        const int base = Wr ? (int)((n0 + h) % Wr) : 0;
        for (int k = tid; k < Wr; k += THREADS) e_ring[(base + k) % Wr] = ehat[h + k];     // bin n0 + h - Wr + k
        if (tid == 0 && (Wr & 1)) e_ring[Wr] = 0.0;                 // the padding to 16 bytes
    }
    {
        uint32_t *ring_out = reinterpret_cast<uint32_t *>(st_out + sizeof(Header) + ring_e);
        // bin r = h - M + k at slot (n0 + r) mod M, k < M: the push's bins from its row, the older ones from state_in (in place
        // they stay where they are).  One flat loop over the ring's 16-byte pieces (or words), so that every lane has work.
        const bool state_quads = (reinterpret_cast<uintptr_t>(a.audio) & 15u) == 0;
        const int per = state_quads ? HOP / 4 : HOP;                // pieces per bin
        const int from = st_out != st_in ? 0 : max(M - h, 0);       // in place: only the push's bins
        for (int at = from * per + tid; at < M * per; at += THREADS) {
            const int k = at / per, i = at % per;
            const int r = h - M + k;
            const int slot = (ring_base + (r % M) + M) % M;
            if (state_quads) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (r >= 0) v = reinterpret_cast<const uint4 *>(push + HOP * r)[i];
                else if (ring_in) v = reinterpret_cast<const uint4 *>(ring_in + HOP * slot)[i];
                reinterpret_cast<uint4 *>(ring_out + HOP * slot)[i] = v;
            } else {
                ring_out[HOP * slot + i] = r >= 0 ? push[HOP * r + i] : (ring_in ? ring_in[HOP * slot + i] : 0u);
            }
        }
    }
}

}  // namespace

LSM_API long lsm_endpoint_state_bytes(int window_bins, int max_bins)
{
    if (window_bins < 1 || window_bins > MAX_WINDOW || max_bins < MIN_SPAN || max_bins > MAX_BINS) return LSM_ERR_ARG;
    return state_bytes(window_bins, max_bins);
}

LSM_API int lsm_endpoint_max_utterances(int n_hops, int hang_bins, int max_bins)
{
    if (n_hops < 1 || n_hops > MAX_HOPS || hang_bins < 1 || hang_bins > MAX_HANG || max_bins < MIN_SPAN || max_bins > MAX_BINS)
        return LSM_ERR_ARG;
    return max_utterances(n_hops, hang_bins, max_bins);
}

LSM_API int lsm_endpoint_stream_f32(const float *audio, int n_streams, int n_hops, const int32_t *stream_hops,
                                    const int32_t *finish, double ratio, double floor, int window_bins, int pad_bins,
                                    int hang_bins, int min_span_bins, int max_bins, const void *state_in, void *state_out,
                                    int max_utts, float *utt_audio_out, int32_t *utt_bins_out, int64_t *utt_first_out,
                                    int32_t *utt_flags_out, int32_t *utt_count_out, double *energy_out, uint8_t *active_out,
                                    void *stream)
{
    LSM_REQUIRE(n_streams >= 0, "n_streams=%d must be >= 0", n_streams);
    LSM_REQUIRE(n_hops >= 1, "n_hops=%d must be >= 1", n_hops);
    if (n_hops > MAX_HOPS) {
        lsm_set_error("n_hops=%d: a push's energies and copy records live in one workgroup's LDS, built for up to %d hops", n_hops,
                      MAX_HOPS);
        return LSM_ERR_UNSUPPORTED;
    }
    LSM_REQUIRE(std::isfinite(ratio) && ratio >= 0.0 && ratio < 1.0, "ratio=%g must be finite and lie in [0, 1)", ratio);
    LSM_REQUIRE(std::isfinite(floor) && floor >= 0.0, "floor=%g must be finite and >= 0", floor);
    LSM_REQUIRE(window_bins >= 1 && window_bins <= MAX_WINDOW, "window_bins=%d outside [1, %d]", window_bins, MAX_WINDOW);
    LSM_REQUIRE(max_bins >= MIN_SPAN && max_bins <= MAX_BINS, "max_bins=%d outside [%d, %d]", max_bins, MIN_SPAN, MAX_BINS);
    LSM_REQUIRE(pad_bins >= 0 && pad_bins < max_bins, "pad_bins=%d outside [0, max_bins=%d)", pad_bins, max_bins);
    LSM_REQUIRE(hang_bins >= (pad_bins > 1 ? pad_bins : 1) && hang_bins <= MAX_HANG,
                "hang_bins=%d outside [max(pad_bins=%d, 1), %d]", hang_bins, pad_bins, MAX_HANG);
    LSM_REQUIRE(min_span_bins >= MIN_SPAN && min_span_bins <= max_bins, "min_span_bins=%d outside [%d, max_bins=%d]",
                min_span_bins, MIN_SPAN, max_bins);
    LSM_REQUIRE(max_utts >= max_utterances(n_hops, hang_bins, max_bins),
                "max_utts=%d is below lsm_endpoint_max_utterances(%d, %d, %d) = %d", max_utts, n_hops, hang_bins, max_bins,
                max_utterances(n_hops, hang_bins, max_bins));
    LSM_REQUIRE(audio && utt_audio_out && utt_bins_out, "endpoint: audio, utt_audio_out and utt_bins_out are required");
    LSM_REQUIRE(utt_audio_out != audio, "utt_audio_out must not be audio");
    LSM_REQUIRE(((uintptr_t)audio & 3u) == 0 && ((uintptr_t)utt_audio_out & 3u) == 0,
                "audio and utt_audio_out must be 4-byte aligned");
    LSM_REQUIRE(((uintptr_t)stream_hops & 3u) == 0 && ((uintptr_t)finish & 3u) == 0 && ((uintptr_t)utt_bins_out & 3u) == 0
                && ((uintptr_t)utt_flags_out & 3u) == 0 && ((uintptr_t)utt_count_out & 3u) == 0,
                "stream_hops, finish, utt_bins_out, utt_flags_out and utt_count_out must be 4-byte aligned");
    LSM_REQUIRE(((uintptr_t)utt_first_out & 7u) == 0 && ((uintptr_t)energy_out & 7u) == 0,
                "utt_first_out and energy_out must be 8-byte aligned");
    LSM_REQUIRE(((uintptr_t)state_in & 15u) == 0 && ((uintptr_t)state_out & 15u) == 0,
                "state_in and state_out must be 16-byte aligned");
    if (n_streams == 0) return LSM_OK;
    EndpointArgs a{};
    a.audio = audio; a.stream_hops = stream_hops; a.finish = finish;
    a.state_in = static_cast<const unsigned char *>(state_in); a.state_out = static_cast<unsigned char *>(state_out);
    a.utt_audio = utt_audio_out; a.utt_bins = utt_bins_out; a.utt_first = utt_first_out; a.utt_flags = utt_flags_out;
    a.utt_count = utt_count_out; a.energy_out = energy_out; a.active_out = active_out;
    a.ratio = ratio; a.floor = floor; a.state_bytes = state_bytes(window_bins, max_bins);
    a.n_hops = n_hops; a.W = window_bins; a.P = pad_bins; a.G = hang_bins; a.A = min_span_bins; a.M = max_bins;
    a.max_utts = max_utts; a.tile_bins = tile_bins_of(n_hops); a.records = records_of(n_hops, max_utts);
    const size_t lds = lds_bytes(n_hops, window_bins, max_utts);
    if (lds > 64 * 1024) lsm_allow_big_lds(reinterpret_cast<const void *>(endpoint_kernel));
    hipLaunchKernelGGL(endpoint_kernel, dim3((unsigned)n_streams), dim3(THREADS), lds, (hipStream_t)stream, a);
    LSM_CHECK_HIP(hipGetLastError());
    return LSM_OK;
}
