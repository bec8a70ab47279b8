// Host check of csrc/endpoint_body.h, the integer arithmetic the endpoint kernel runs its state machine and addresses memory
// with: built with -fsanitize=address,undefined and run by tests/test_endpoint_host.py.  It drives the machine against a table
// of hand cases, checks that a run cut into two launches through a stored header is the uncut run, and replays a launch's
// addressing -- clamped hops, ring residues, utterance slots -- in heap buffers of exactly the launch's sizes from headers that
// hold anything an int64 can: an index outside a buffer, or an overflowing sum, ends the run.
#include "endpoint_body.h"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace lsm_endpoint;

struct Utt {
    long long first;
    int bins, flags;
    bool kept;
    bool operator==(const Utt &o) const { return first == o.first && bins == o.bins && flags == o.flags && kept == o.kept; }
};

static long checked = 0;

static void fail(const char *what, const char *detail)
{
    std::printf("FAIL %s: %s\n", what, detail);
    std::exit(1);
}

// One launch on a header: activity '1' / '0' per bin; every close is reported with its absolute first bin.
static void launch(Header &hd, const std::string &act, bool fin, int P, int G, int A, int M, std::vector<Utt> &out)
{
    const int64_t n0 = first_bin(hd);
    Machine m = load(hd, G, M);
    Closed c;
    const int h = (int)act.size();
    for (int j = 0; j < h; ++j)
        if (step(m, j, act[(size_t)j] == '1', P, G, A, M, c)) out.push_back(Utt{n0 + c.s, c.bins, c.flags, c.kept});
    if (fin && finish(m, h, P, A, c)) out.push_back(Utt{n0 + c.s, c.bins, c.flags, c.kept});
    if (fin) std::memset(&hd, 0, sizeof hd);
    else store(m, n0, h, hd);
}

static void hand(const char *name, const std::string &act, bool fin, int P, int G, int A, int M, const std::vector<Utt> &want)
{
    std::vector<Utt> whole;
    Header hd{};
    launch(hd, act, fin, P, G, A, M, whole);
    if (!(whole == want)) {
        for (const Utt &u : whole) std::printf("  got first=%lld bins=%d flags=%d kept=%d\n", u.first, u.bins, u.flags, (int)u.kept);
        fail("hand case", name);
    }
    // every split into two launches, and bin by bin, through the stored header
    for (size_t cut = 0; cut <= act.size(); ++cut) {
        std::vector<Utt> parts;
        Header h2{};
        launch(h2, act.substr(0, cut), false, P, G, A, M, parts);
        launch(h2, act.substr(cut), fin, P, G, A, M, parts);
        if (!(parts == want)) fail("split", name);
    }
    std::vector<Utt> single;
    Header h3{};
    for (size_t j = 0; j < act.size(); ++j) launch(h3, act.substr(j, 1), false, P, G, A, M, single);
    launch(h3, "", fin, P, G, A, M, single);
    if (!(single == want)) fail("bin by bin", name);
    ++checked;
}

// A launch's addressing, as endpoint.hip forms it, in buffers of the launch's sizes.
static void addressing(Header hd, int n_hops, int hops_value, bool fin, unsigned seed, int W, int P, int G, int A, int M)
{
    const int max_utts = max_utterances_padded(n_hops, P, G, M);
    const int Wr = W - 1;
    std::vector<unsigned char> state((size_t)state_bytes(W, M), 0), state_out((size_t)state_bytes(W, M), 0);
    std::vector<float> audio((size_t)n_hops * HOP, 1.0f), slots((size_t)max_utts * HOP * M, -1.0f);
    std::vector<double> ehat((size_t)(Wr + n_hops), 0.0);
    std::memcpy(state.data(), &hd, sizeof hd);
    const int h = clamp_hops(hops_value, n_hops);
    if (h < 0 || h > n_hops) fail("clamp_hops", "outside [0, n_hops]");
    const int64_t n0 = first_bin(hd);
    const double *e_ring = reinterpret_cast<const double *>(state.data() + sizeof(Header));
    const int e_base = Wr ? (int)(n0 % Wr) : 0;
    for (int k = 0; k < Wr; ++k)
        if (n0 - Wr + k >= 0) ehat[(size_t)k] = e_ring[(e_base + k) % Wr];
    Machine m = load(hd, G, M);
    if (m.avail > 0 || m.avail < -M) fail("load", "avail");
    if (m.mode == SPEECH && !(-(M - 1) <= m.s && m.s <= m.f && m.f <= m.last && m.last <= -1 && -m.last <= G)) fail("load", "open");
    const float *ring = reinterpret_cast<const float *>(state.data() + sizeof(Header) + energy_ring_bytes(W));
    float *ring_out = reinterpret_cast<float *>(state_out.data() + sizeof(Header) + energy_ring_bytes(W));
    const int ring_base = (int)(n0 % M);
    int count = 0;
    unsigned lcg = seed;
    Closed c;
    auto emit = [&](const Closed &u) {
        if (!u.kept) return;
        if (count >= max_utts) fail("closure bound", "more kept utterances than max_utterances_padded");
        if (u.bins < 1 || u.bins > M || u.s <= -M || u.s + u.bins > h) fail("utterance", "outside the ring and the push");
        if (u.bins < MIN_SPAN) fail("utterance", "kept with fewer than 3 bins");
        float *row = slots.data() + (size_t)count * HOP * M;
        for (int k = 0; k < u.bins; ++k) {
            const int r = u.s + k;
            const float *src = r >= 0 ? audio.data() + (size_t)HOP * r : ring + (size_t)HOP * ((ring_base + r + M) % M);
            for (int i = 0; i < HOP; ++i) row[HOP * k + i] = src[i];
        }
        for (int i = HOP * u.bins; i < HOP * M; ++i) row[i] = 0.0f;
        ++count;
    };
    for (int j = 0; j < h; ++j) {
        lcg = lcg * 1664525u + 1013904223u;
        const bool on = seed == 0 ? true : seed == 1 ? false : (lcg >> 16) % 3 != 0;
        ehat[(size_t)(Wr + j)] = on ? 1.0 : 0.0;
        if (step(m, j, on, P, G, A, M, c)) emit(c);
    }
    if (fin && finish(m, h, P, A, c)) emit(c);
    Header next;
    store(m, n0, h, next);
    if (next.n != n0 + h) fail("store", "n");
    double *e_out = reinterpret_cast<double *>(state_out.data() + sizeof(Header));
    const int e_next = Wr ? (int)((n0 + h) % Wr) : 0;
    for (int k = 0; k < Wr; ++k) e_out[(e_next + k) % Wr] = ehat[(size_t)(h + k)];
    for (int k = 0; k < M; ++k) {
        const int r = h - M + k;
        const int slot = (ring_base + (r % M) + M) % M;
        const float *src = r >= 0 ? audio.data() + (size_t)HOP * r : ring + (size_t)HOP * slot;
        for (int i = 0; i < HOP; ++i) ring_out[(size_t)HOP * slot + i] = src[i];
    }
    ++checked;
}

int main()
{
    // one word closes at last + P; the pre-roll stops at the stream's start
    hand("word", "0011100000", false, 1, 2, 3, 20, {{1, 5, 0, true}});
    hand("pre-roll at the start", "0111000000", false, 3, 3, 3, 20, {{0, 7, 0, true}});
    // the pre-roll of a second word stops at avail = end + 1 of the first
    hand("pre-roll at avail", "111000111000", false, 2, 3, 3, 20, {{0, 5, 0, true}, {5, 6, 0, true}});
    // a click shorter than A is dropped, and its bins are taken (avail moves)
    hand("click", "0010000", false, 0, 2, 3, 20, {{2, 1, 0, false}});
    // a word longer than M: M bins with bit 0, then the rest
    hand("forced cut", "11111111100", false, 0, 2, 3, 6, {{0, 6, FLAG_CUT, true}, {6, 3, 0, true}});
    // n - last == G wins over the length check on the same bin
    hand("hang before length", "11100", false, 0, 2, 3, 5, {{0, 3, 0, true}});
    // finish while open (end stops at the last bin seen) and while idle
    hand("finish open", "0111", true, 2, 4, 3, 20, {{0, 4, FLAG_FLUSHED, true}});
    hand("finish open, short", "01", true, 0, 4, 3, 20, {{1, 1, FLAG_FLUSHED, false}});
    hand("finish idle", "0000", true, 2, 4, 3, 20, {});
    // P = M - 1: a word that starts late is cut at once
    hand("cut by pre-roll", "00001", false, 3, 3, 3, 4, {{1, 4, FLAG_CUT, true}});

    // the bound's figures
    if (max_utterances(1, 1, 3) != 2 || max_utterances(100, 20, 100) != 6 || max_utterances(4096, 1, 3) != 2049
        || max_utterances(65, 4, 3) != 23)
        fail("max_utterances", "figures");
    if (closure_spacing(3, 20, 100) != 21 || closure_spacing(5, 10, 13) != 8 || closure_spacing(0, 10, 13) != 11
        || closure_spacing(10, 10, 13) != 11 || closure_spacing(2, 4, 5) != 5)
        fail("closure_spacing", "figures");
    if (state_bytes(1, 3) != 64 + 1920 || state_bytes(2, 3) % 16 || state_bytes(1024, 4096) % 16) fail("state_bytes", "figures");

    // headers that hold anything, counts that hold anything
    const int64_t values[] = {0, 1, -1, 7, 1000, INT64_MIN, INT64_MAX, ((int64_t)1 << 62) + 3};
    const int shapes[][6] = {{7, 1, 0, 1, 3, 3}, {7, 8, 3, 4, 3, 12}, {64, 2, 2, 2, 3, 3}, {65, 8, 0, 4, 3, 12}, {30, 5, 5, 10, 3, 13},
                             {1, 3, 11, 11, 12, 12}};
    for (const auto &sh : shapes) {
        unsigned seed = 0;
        for (int64_t n : values)
            for (int64_t s : values)
                for (int64_t last : values)
                    for (int mode : {0, 1, 2, INT_MIN}) {
                        Header hd{};
                        hd.n = n; hd.s = s; hd.f = last ^ 1; hd.last = last; hd.avail = s ^ n; hd.mode = mode;
                        for (int hops : {sh[0], 0, sh[0] + 5, INT_MIN, INT_MAX})
                            addressing(hd, sh[0], hops, (seed & 4) != 0, seed % 5, sh[1], sh[2], sh[3], sh[4], sh[5]);
                        ++seed;
                    }
    }
    // the closure bound over random activity from a fresh stream, wide shapes included
    for (unsigned seed = 2; seed < 400; ++seed) {
        const int G = 1 + (int)(seed * 7u % 12u), M = 3 + (int)(seed * 13u % 14u);
        const int P = (int)(seed * 5u % (unsigned)((G < M - 1 ? G : M - 1) + 1));
        addressing(Header{}, 1 + (int)(seed * 31u % 300u), INT_MAX, (seed & 1) != 0, seed, 1 + (int)(seed % 9u), P, G, 3, M);
    }
    std::printf("endpoint_body ok: %ld cases\n", checked);
    return 0;
}
