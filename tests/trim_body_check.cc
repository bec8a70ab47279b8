// Host check of csrc/trim_body.h, the integer arithmetic the trim kernel addresses memory with: built with
// -fsanitize=address,undefined and run by tests/test_trim_host.py.  For every combination of the count corners it forms
// the clip's length, bins, span and copied samples exactly as the kernel does and touches, in heap buffers of exactly the
// launch's sizes, every element the kernel would touch: an index outside a buffer, or an overflowing sum, ends the run.
#include "trim_body.h"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace lsm_trim;

static long checked = 0;

static void fail(const char *what, int n_samples, int time_bins, int count, int fa, int la, int pad, int minb)
{
    std::printf("FAIL %s: n_samples=%d time_bins=%d count=%d active=[%d,%d] pad=%d min=%d\n", what, n_samples, time_bins, count, fa,
                la, pad, minb);
    std::exit(1);
}

static void one(int n_samples, int time_bins, int extra_out, int count, int fa, int la, bool whole, int pad, int minb)
{
    const int n_out = HOP * time_bins + extra_out;
    std::vector<float> in((size_t)n_samples, 1.0f), out((size_t)n_out, -1.0f);
    std::vector<double> energy((size_t)time_bins, -1.0);
    float *src = in.data(), *dst = out.data();
    const int len = clamp_len(count, n_samples);
    const int nb = bins_of(len, time_bins);
    if (len < 0 || len > n_samples || nb < 0 || nb > time_bins) fail("clamp", n_samples, time_bins, count, fa, la, pad, minb);
    if ((long long)nb * HOP < len && nb < time_bins) fail("bins", n_samples, time_bins, count, fa, la, pad, minb);
    // energies: the staged reads and the energy rows
    volatile float sink = 0.0f;
    for (int at = 0; at < HOP * nb; ++at)
        if (at < len) sink = sink + src[at];
    for (int j = 0; j < nb; ++j) energy[(size_t)j] = 0.0;
    if (nb >= 1) {
        fa = fa < nb ? fa : nb - 1;
        la = la < nb ? la : nb - 1;
        if (la < fa) la = fa;
    }
    const Span s = endpoints(nb, whole || nb < 1, fa, la, pad, minb);
    if (s.first < 0 || s.bins < 0 || s.first + s.bins > nb) fail("span", n_samples, time_bins, count, fa, la, pad, minb);
    if (!whole && nb >= MIN_BINS) {
        const int m = minb < nb ? minb : nb;
        if (s.bins < m || s.first > fa || s.first + s.bins - 1 < la) fail("rule", n_samples, time_bins, count, fa, la, pad, minb);
    } else if (s.first != 0 || s.bins != nb) {
        fail("whole", n_samples, time_bins, count, fa, la, pad, minb);
    }
    const int valid = copied_samples(len, s);
    if (valid < 0 || valid > HOP * s.bins || valid > n_out) fail("valid", n_samples, time_bins, count, fa, la, pad, minb);
    for (int m = 0; m < valid; ++m) dst[m] = src[HOP * s.first + m];
    for (int m = valid; m < n_out; ++m) dst[m] = 0.0f;
    ++checked;
}

int main()
{
    const int bins_set[] = {3, 4, 7, 100};
    for (int time_bins : bins_set) {
        const int samples_set[] = {1, 321, HOP * time_bins - 1, HOP * time_bins, HOP * time_bins + 7};
        for (int n_samples : samples_set) {
            const int counts[] = {0, 1, 159, 160, 161, 320, 321, n_samples - 1, n_samples, n_samples + 1, -1, INT_MIN, INT_MAX};
            for (int count : counts)
                for (int pad : {0, 1, 3, time_bins, INT_MAX})
                    for (int minb : {3, time_bins})
                        for (int fa = 0; fa < time_bins; fa += (time_bins > 8 ? 33 : 1))
                            for (int la = fa; la < time_bins; la += (time_bins > 8 ? 33 : 1)) {
                                one(n_samples, time_bins, 0, count, fa, la, false, pad, minb);
                                one(n_samples, time_bins, 5, count, fa, time_bins - 1, false, pad, minb);
                            }
            for (int count : counts) one(n_samples, time_bins, 3, count, 0, 0, true, 2, 3);
        }
    }
    // the top of the range, and a row as long as an int allows counted in full
    one(HOP * MAX_BINS, MAX_BINS, 0, INT_MAX, 0, MAX_BINS - 1, false, INT_MAX, MAX_BINS);
    one(HOP * MAX_BINS + 1, MAX_BINS, 1, HOP * MAX_BINS + 1, MAX_BINS - 1, MAX_BINS - 1, false, 0, 3);
    if (clamp_len(INT_MAX, INT_MAX) != INT_MAX || bins_of(INT_MAX, MAX_BINS) != MAX_BINS) return 1;
    std::printf("trim_body ok: %ld cases\n", checked);
    return 0;
}
