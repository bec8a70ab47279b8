// Stream endpointing (SPEC.md §1.17, include/lsm_hip_endpoint.h): the integer arithmetic of a stream -- the layout of its
// state block, the clamps of what a block and a count array may hold, the state machine of one bin, the finish and the closure
// bound -- as host and device code, one copy: the kernel (endpoint.hip) and a host program (tests/endpoint_body_check.cc)
// compile this file.  Nothing here reads memory.
//
// The machine works in bins RELATIVE to the first bin of the launch: r = n - n0, so -M < r < n_hops and every value fits an
// int whatever the 64-bit bin counter of the stream holds.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LSM_ENDPOINT_HD __host__ __device__
#else
#define LSM_ENDPOINT_HD
#endif

namespace lsm_endpoint {

constexpr int HOP = 160;            // samples per bin (frontend.RAGGED_HOP)
constexpr int MAX_HOPS = 4096;      // n_hops of a launch: 1 .. 4096
constexpr int MAX_WINDOW = 1024;    // window_bins: 1 .. 1024
constexpr int MAX_HANG = 1024;      // hang_bins: max(pad_bins, 1) .. 1024
constexpr int MIN_SPAN = 3;         // min_span_bins and max_bins: >= 3 (a ragged clip has at least 3 bins)
constexpr int MAX_BINS = 4096;      // max_bins: 3 .. 4096
constexpr int FLAG_CUT = 1, FLAG_FLUSHED = 2;
constexpr int IDLE = 0, SPEECH = 1;

// The state block: this header, the last W - 1 values of e^ (bin i at slot i mod (W - 1), padded to 16 bytes), the last M bins
// of audio (bin i at slot i mod M, 160 words each).  All zeros is a fresh stream.
struct Header {
    int64_t n;                      // bins seen since the stream's start
    int64_t s, f, last;             // the open utterance: first bin, first and last active bin (SPEECH only, else 0)
    int64_t avail;                  // the first bin a new utterance may take
    int32_t mode;
    int32_t reserved[5];
};
static_assert(sizeof(Header) == 64, "the header is 64 bytes");

LSM_ENDPOINT_HD inline long energy_ring_bytes(int W)
{
    return (8L * (W - 1) + 15) / 16 * 16;
}

LSM_ENDPOINT_HD inline long state_bytes(int W, int M)
{
    return (long)sizeof(Header) + energy_ring_bytes(W) + 4L * HOP * M;
}

// h_b: any int32 -> 0 .. n_hops
LSM_ENDPOINT_HD inline int clamp_hops(int v, int n_hops)
{
    return v < 0 ? 0 : (v > n_hops ? n_hops : v);
}

// What lsm_endpoint_max_utterances returns (1 <= H, 1 <= G, 3 <= M): 2 + (H - 1) / min(G + 1, M).
LSM_ENDPOINT_HD inline int max_utterances(int H, int G, int M)
{
    const int d = G + 1 < M ? G + 1 : M;
    return 2 + (H - 1) / d;
}

// The fewest bins between the closes of two KEPT utterances: a close by silence needs an active bin and G quiet ones behind
// the previous close, a forced cut behind a forced cut M bins, and a forced cut behind a close by silence (avail = c - G + P + 1,
// first active bin >= c + 1) max(M - P, M + P - G) bins.  The last term is below min(G + 1, M) only where G + 3 <= M (a kept
// utterance can close by silence at all) and M - G - 1 < P < 2 G + 1 - M.
LSM_ENDPOINT_HD inline int closure_spacing(int P, int G, int M)
{
    int d = G + 1 < M ? G + 1 : M;
    if (G + 3 <= M) {
        const int after_silence = M - P > M + P - G ? M - P : M + P - G;
        if (after_silence < d) d = after_silence;
    }
    return d;
}

// The slots no push of H hops can exceed whatever pad_bins is: 2 + (H - 1) / closure_spacing.  Equal to max_utterances wherever
// closure_spacing is min(G + 1, M).
LSM_ENDPOINT_HD inline int max_utterances_padded(int H, int P, int G, int M)
{
    return 2 + (H - 1) / closure_spacing(P, G, M);
}

struct Machine {
    int s, f, last, avail, mode;    // relative bins
};

struct Closed {
    int s, bins, flags;
    bool kept;
};

LSM_ENDPOINT_HD inline int clamp_rel(int64_t v, int64_t n0, int lo, int hi)
{
    const int64_t d = (int64_t)((uint64_t)v - (uint64_t)n0);       // wraps instead of overflowing; clamped next
    return d < lo ? lo : (d > hi ? hi : (int)d);
}

// n0 of a block: a counter below 0 or near the end of int64 (no stream gets there: a block from elsewhere) is clamped
LSM_ENDPOINT_HD inline int64_t first_bin(const Header &h)
{
    const int64_t top = (int64_t)1 << 62;
    return h.n < 0 ? 0 : (h.n > top ? top : h.n);
}

// A block's integers as the machine of this launch.  Every clamp is the identity on a block this code wrote under the same
// G, M: an open utterance has 1 .. M - 1 bins, s <= f <= last, fewer than G quiet bins behind last; avail <= n0.
LSM_ENDPOINT_HD inline Machine load(const Header &h, int G, int M)
{
    const int64_t n0 = first_bin(h);
    Machine m;
    m.mode = h.mode == SPEECH ? SPEECH : IDLE;
    m.avail = clamp_rel(h.avail, n0, -M, 0);
    if (m.mode == SPEECH) {
        m.s = clamp_rel(h.s, n0, -(M - 1), -1);
        const int quiet = -G > m.s ? -G : m.s;
        m.last = clamp_rel(h.last, n0, quiet, -1);
        m.f = clamp_rel(h.f, n0, m.s, m.last);
    } else {
        m.s = m.f = m.last = 0;
    }
    return m;
}

// The block's integers after a launch of h bins
LSM_ENDPOINT_HD inline void store(const Machine &m, int64_t n0, int h, Header &out)
{
    const bool open = m.mode == SPEECH;
    out.n = n0 + h;
    out.s = open ? n0 + m.s : 0;
    out.f = open ? n0 + m.f : 0;
    out.last = open ? n0 + m.last : 0;
    out.avail = n0 + m.avail;
    out.mode = m.mode;
    for (int i = 0; i < 5; ++i) out.reserved[i] = 0;
}

LSM_ENDPOINT_HD inline void close(Machine &m, int end, int flags, int A, Closed &c)
{
    c.s = m.s;
    c.bins = end - m.s + 1;
    c.flags = flags;
    c.kept = (flags & FLAG_CUT) != 0 || m.last - m.f + 1 >= A;
    m.avail = end + 1;
    m.mode = IDLE;
    m.s = m.f = m.last = 0;
}

// Bin n (relative) with its activity.  True when an utterance closed on this bin: `c` says which and whether it is kept.
// 0 <= P < M, max(P, 1) <= G, 3 <= A <= M.  `>=` where the rule says `==`: the same on every reachable state.
LSM_ENDPOINT_HD inline bool step(Machine &m, int n, bool active, int P, int G, int A, int M, Closed &c)
{
    if (m.mode == IDLE) {
        if (!active) return false;
        m.s = n - P > m.avail ? n - P : m.avail;
        m.f = m.last = n;
        m.mode = SPEECH;
    } else if (active) {
        m.last = n;
    }
    if (n - m.last >= G) {
        close(m, m.last + P, 0, A, c);          // P <= G: end <= n
        return true;
    }
    if (n - m.s + 1 >= M) {
        close(m, n, FLAG_CUT, A, c);
        return true;
    }
    return false;
}

// The stream ends behind bin h - 1 (relative; h = 0: behind the bins of earlier launches).  True when an utterance was open.
LSM_ENDPOINT_HD inline bool finish(Machine &m, int h, int P, int A, Closed &c)
{
    if (m.mode != SPEECH) return false;
    const int end = m.last + P < h - 1 ? m.last + P : h - 1;
    close(m, end, FLAG_FLUSHED, A, c);
    return true;
}

}  // namespace lsm_endpoint
