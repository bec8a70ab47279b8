"""CPU check of the pair-block kernel's input tables (csrc/lif_pair.h, csrc/reservoir.hip: colour_input_channels,
pair_input_words).  `lsm_debug_pair_inputs` is host arithmetic only -- the functions lsm_reservoir_create uses -- and returns
the bit position of every channel in a step's input bit row plus the four words per neuron the kernel holds in registers:
up to 128 channels the channel masks, from 129 to 256 channels {posmask, P0, P1, P2} (one (position -> row word) entry per
coloured bit).  Reference: the input map itself (SPEC.md 2.4, 3: the input term of neuron i is w_in times the number of
spiking channels among the entries that name i); the words are decoded back into (channel, neuron) pairs, and the kernel's
count -- restated in NumPy exactly as it is computed, seven bitwise selects, one and, one popcount -- is compared with the
count taken from the map.  Everything is integers: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from lsm_speech_classifier_amd import _lib, reservoir as R

WIDE = (129, 160, 200, 256)
NARROW = (96, 128)
N, K = 1024, 60


def _map(c, n=N):
    res = R.build_reservoir(R.SimulationParams(num_neurons=n, num_output_neurons=n // 3, small_world_graph_k=K,
                                               mean_weight=0.004), c)
    return np.ascontiguousarray(res.in_tgt, dtype=np.int32)


def _hub_map(c, hub_channels, n=N, fan=5):
    """The first `hub_channels` channels all feed neuron 0; every (channel, neuron) pair occurs once."""
    rs = np.random.RandomState(hub_channels)
    in_tgt = np.empty((c, fan), dtype=np.int32)
    for ch in range(c):
        others = rs.choice(np.arange(1, n), fan - 1, replace=False)
        first = 0 if ch < hub_channels else int(rs.randint(1, n))
        while first in others:
            first = int(rs.randint(1, n))
        in_tgt[ch] = np.sort(np.append(others, first))
    return in_tgt


def _tables(in_tgt, n=N, wpc=4):
    lib = _lib.load()
    c, fan = in_tgt.shape
    npad = 256 * ((n + 255) // 256)
    perm = np.full(c, 255, dtype=np.uint8)
    words = np.full((npad, 4), 0xFFFFFFFF, dtype=np.uint32)
    in_tgt = np.ascontiguousarray(in_tgt, dtype=np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    form = lib.lsm_debug_pair_inputs(n, c, p(in_tgt), fan, wpc, p(perm), p(words))
    assert form >= 0, lib.lsm_last_error()
    assert lib.lsm_debug_pair_inputs(n, c, p(in_tgt), fan, wpc, None, None) == form      # the form alone
    return form, perm.astype(np.int64), words


def _pairs_of(in_tgt):
    return sorted((ch, int(i)) for ch in range(in_tgt.shape[0]) for i in in_tgt[ch])


def _decode(form, perm, words, c):
    """(channel, neuron) pairs the words stand for."""
    chan_at = {int(p): ch for ch, p in enumerate(perm)}
    out = []
    for i in np.nonzero(words.any(axis=1))[0]:
        w = [int(x) for x in words[i]]
        if form == 3:
            assert not (w[1] | w[2] | w[3]) & ~w[0], "a plane bit without its position bit"
            for p in range(32):
                if (w[0] >> p) & 1:
                    word = ((w[1] >> p) & 1) | (((w[2] >> p) & 1) << 1) | (((w[3] >> p) & 1) << 2)
                    out.append((chan_at[word * 32 + p], int(i)))
        else:
            for pos in range(128):
                if (w[pos >> 5] >> (pos & 31)) & 1:
                    out.append((chan_at[pos], int(i)))
    assert all(0 <= ch < c for ch, _ in out)
    return sorted(out)


def _bfi(s, a, b):
    return (s & a) | (~s & b)


def _popcount(x):
    return np.unpackbits(np.ascontiguousarray(x, dtype=np.uint32).view(np.uint8)).reshape(len(x), 32).sum(axis=1)


def _kernel_count(form, words, d):
    """What lif_pair.h computes per neuron from its four words and the step's row words d[0..7]."""
    w = [words[:, k] for k in range(4)]
    if form == 3:
        a = [_bfi(w[1], d[2 * q + 1], d[2 * q]) for q in range(4)]
        b = [_bfi(w[2], a[1], a[0]), _bfi(w[2], a[3], a[2])]
        return _popcount(_bfi(w[3], b[1], b[0]) & w[0])
    return sum(_popcount(w[k] & d[k]) for k in range(4))


def _reference_positions(n, in_tgt):
    """The documented assignment (csrc/reservoir.hip, colour_input_channels), restated: channels conflict when they share a
    target; by descending conflict degree (ties: channel order) a channel takes, among the 32 colours free of its coloured
    neighbours and not yet holding ceil(C/32) channels, the emptiest (ties: the lowest); when none is left, one member of a
    colour free of its neighbours moves to another colour it may take.  The members of a colour get the words 0, 1, ... in
    channel order.  None when no assignment is found."""
    c = in_tgt.shape[0]
    cap = (c + 31) // 32
    chans_of = [[] for _ in range(n)]
    for ch in range(c):
        for i in in_tgt[ch]:
            chans_of[i].append(ch)
    adj = np.zeros((c, c), dtype=bool)
    for l in chans_of:
        for x in l:
            for y in l:
                if x != y:
                    adj[x, y] = True
    deg = adj.sum(axis=1)
    order = sorted(range(c), key=lambda x: -deg[x])                  # stable
    col, cnt = [-1] * c, [0] * 32

    def used_by_neighbours(x):
        return {col[y] for y in np.nonzero(adj[x])[0] if col[y] >= 0}

    for x in order:
        used = used_by_neighbours(x)
        best = -1
        for k in range(32):
            if k not in used and cnt[k] < cap and (best < 0 or cnt[k] < cnt[best]):
                best = k
        if best < 0:
            for k in range(32):
                if best >= 0 or k in used:
                    continue
                for v in range(c):
                    if best >= 0 or col[v] != k:
                        continue
                    uv = used_by_neighbours(v)
                    for q in range(32):
                        if q != k and q not in uv and cnt[q] < cap and not adj[v, x]:
                            col[v] = q; cnt[q] += 1; cnt[k] -= 1
                            best = k
                            break
            if best < 0:
                return None
        col[x] = best
        cnt[best] += 1
    nxt = [0] * 32
    perm = np.zeros(c, dtype=np.int64)
    for ch in range(c):
        perm[ch] = nxt[col[ch]] * 32 + col[ch]
        nxt[col[ch]] += 1
    return perm


@pytest.mark.parametrize("c", WIDE + NARROW)
def test_the_words_are_the_input_map(c):
    in_tgt = _map(c)
    form, perm, words = _tables(in_tgt)
    assert form == (3 if c > 128 else 2)                             # the builder's maps have a colouring
    cw = (c + 31) // 32
    # positions: a permutation into [0, 32 * ceil(C/32)); channels sharing a neuron differ mod 32
    assert len(set(perm.tolist())) == c and perm.min() >= 0 and perm.max() < 32 * cw
    for i in range(N):
        chans = np.nonzero((in_tgt == i).any(axis=1))[0]
        assert len(set((perm[chans] % 32).tolist())) == len(chans), i
    assert not words[N:].any()                                       # padding neurons have no inputs
    assert _decode(form, perm, words, c) == _pairs_of(in_tgt)
    # the kernel's count against the count taken from the map, 40 random rows (plus none and all)
    rs = np.random.RandomState(c)
    rows = [np.zeros(c, bool), np.ones(c, bool)] + [rs.rand(c) < rs.uniform(0.05, 0.9) for _ in range(40)]
    for spiking in rows:
        d = np.zeros(8, dtype=np.uint32)
        for ch in np.nonzero(spiking)[0]:
            d[perm[ch] >> 5] |= np.uint32(1 << (perm[ch] & 31))
        want = np.zeros(words.shape[0], dtype=np.int64)
        np.add.at(want, in_tgt[spiking].reshape(-1), 1)
        np.testing.assert_array_equal(_kernel_count(form, words, d), want)
        if form == 3 and cw < 8:
            # the kernel does not clear the row words past ceil(C/32): whatever they hold must not count
            d[cw:] = rs.randint(0, 2 ** 32, size=8 - cw, dtype=np.uint64).astype(np.uint32)
            np.testing.assert_array_equal(_kernel_count(form, words, d), want)


@pytest.mark.parametrize("c", NARROW + (160,))
def test_positions_are_the_documented_assignment(c):
    """Up to 128 channels the dense kernel's mode 3 and the ring modes 13 / 15 read the same positions: widening the
    assignment to 256 channels must not move them.  The words are then the four channel masks at those positions."""
    in_tgt = _map(c)
    form, perm, words = _tables(in_tgt, wpc=8)
    want = _reference_positions(N, in_tgt)
    assert want is not None
    np.testing.assert_array_equal(perm, want)
    if c <= 128:
        assert form == 2
        masks = np.zeros((words.shape[0], 4), dtype=np.uint32)
        for ch in range(c):
            for i in in_tgt[ch]:
                masks[i, want[ch] >> 5] |= np.uint32(1 << (want[ch] & 31))
        np.testing.assert_array_equal(words, masks)


def test_natural_positions_without_a_colouring_up_to_128_channels():
    in_tgt = _hub_map(96, 33)
    form, perm, words = _tables(in_tgt)
    assert form == 1
    np.testing.assert_array_equal(perm, np.arange(96))
    assert _decode(form, perm, words, 96) == _pairs_of(in_tgt)


def test_maps_without_a_form():
    lib = _lib.load()
    assert _tables(_hub_map(160, 33))[0] == 0                        # 33 channels onto one neuron: no 32-colouring
    form, perm, words = _tables(_hub_map(160, 32))                   # 32: the tightest map that has one
    assert form == 3 and len(set((perm[:32] % 32).tolist())) == 32
    assert _decode(form, perm, words, 160) == _pairs_of(_hub_map(160, 32))
    for c in (96, 160):
        twice = _map(c).copy()
        twice[3, 1] = twice[3, 0]                                    # a channel that lists a neuron twice
        assert _tables(twice)[0] == 0
    assert _tables(_map(257))[0] == 0
    assert _tables(_map(160), wpc=16)[0] == 0                        # 8 blocks do not share out over 16 waves
    in_tgt = _map(160)
    assert lib.lsm_debug_pair_inputs(N, 160, C.c_void_p(in_tgt.ctypes.data), in_tgt.shape[1], 5, None, None) < 0
