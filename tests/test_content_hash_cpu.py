"""sgl_content_hash on the CPU (the function is host-only): it is the key of three caches -- the shims' cached adjacency, AdjIdentity and
the on-disk hop cache -- so a collision is a cache hit that returns another input's result.  The library against a serial restatement
of the header text at every length where the code takes another path, and families of edits that must never collide: for a sound
64-bit hash the expected number of collisions at these trial counts is below 1e-10, so the allowed number is 0.

Until this file the per-word step was a bare multiply; a difference in the top bits of a word stayed there for the rest of its lane,
and two sign flips in one lane cancelled: family (a) collided in 480 of 480 float64 pairs and 112 of 480 float32 pairs."""
import numpy as np
import pytest
import torch

import content_hash_common as chc
from sgl_amd import _lib


@pytest.mark.parametrize("nbytes", chc.LENGTHS)
def test_library_equals_the_serial_restatement(nbytes):
    """the library runs with the machine's team of threads, the restatement with one: equality also shows that the result does
    not depend on the team size.  The same bytes at a source that is only 1-byte aligned give the same value."""
    room = chc.seeded_bytes(nbytes + 1, seed=nbytes % 1009)
    buf = room[1:]
    assert (nbytes == 0 or buf.ctypes.data % 2 == 1) and buf.flags.c_contiguous       # 1-byte aligned: memcpy loads only
    want = chc.serial_hash(buf)
    assert _lib.content_hash(buf) == want
    aligned = buf.copy()
    assert aligned.ctypes.data % 8 == 0 and _lib.content_hash(aligned) == want
    if nbytes:
        assert want != chc.serial_hash(buf[:-1]) and _lib.content_hash(buf[:-1]) == chc.serial_hash(buf[:-1])


def test_restatement_reads_as_the_header_does():
    """the constants of tests/content_hash_common.py are the ones of the text at sgl_content_hash in include/sgl_hip.h"""
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "sgl_hip.h")).read()
    text = text[text.index("order-sensitive 64-bit hash of a HOST buffer"):text.index("int sgl_content_hash(")]
    for c in (chc.M1, chc.M2, *chc.LANE_SEEDS, chc.FOLD_SEED, chc.TOTAL_SEED):
        assert f"0x{c:016X}" in text, hex(c)
    assert "t >> 64" in text and "128-bit product" in text and "2^20 bytes" in text and "32-byte groups" in text and "lane 0 alone" in text
    assert (chc.BLOCK, chc.GROUP) == (1 << 20, 32)
    # and a value nobody computed with the library: the empty buffer is fmix(seed ^ 0)
    assert chc.serial_hash(np.zeros(0, np.uint8)) == chc.fmix(chc.TOTAL_SEED) == _lib.content_hash(np.zeros(0, np.uint8))


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
def test_paired_sign_flips_never_collide(dtype):
    """(a) exhaustive: every pair of same-lane positions of a 64-element buffer, both negated"""
    hits, trials = chc.paired_sign_flips(_lib.content_hash, dtype)
    assert trials == 480 and hits == 0, (hits, trials)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_paired_rescalings_never_collide(dtype):
    """(b) two same-lane values each multiplied by 2^k, k in [-6, 6]: only exponent bits move"""
    hits, trials = chc.paired_rescalings(_lib.content_hash, dtype)
    assert trials == 20_000 and hits == 0, (hits, trials)


@pytest.mark.parametrize("words", [2, 3])
def test_top_bit_masks_never_collide(words):
    """(c) xor masks confined to the top k bits of 2 and of 3 words of one lane, k = 1 .. 16"""
    bad = {}
    for k in range(1, 17):
        hits, trials = chc.top_bit_masks(_lib.content_hash, k, words)
        assert trials == 2_000
        if hits:
            bad[k] = hits
    assert not bad, bad


@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.float64])
@pytest.mark.parametrize("words", [2, 3])
def test_sign_flips_in_a_window_of_one_lane_never_collide(dtype, words):
    """exhaustive: every non-empty subset of sign flips over the elements of 2 and of 3 consecutive words of one lane.  A step that
    leaves a flipped sign bit as a fixed pattern in the lane (multiply, then t ^ t >> 32: bits 63 and 31) collides here whenever
    the next word's flips are that pattern -- val[[1, 8, 9]] *= -1 -- in every buffer"""
    hits, trials = chc.window_sign_flips(_lib.content_hash, dtype, words)
    per = 8 // np.dtype(dtype).itemsize
    assert trials == 40 * ((1 << words * per) - 1) and hits == 0, (hits, trials)


@pytest.mark.parametrize("words", [2, 3])
def test_masks_on_both_halves_never_collide(words):
    """top-k-bit masks on both 32-bit halves of 2 and of 3 words of one lane (adjacent in every other trial), k = 1 .. 16"""
    bad = {}
    for k in range(1, 17):
        hits, trials = chc.both_half_masks(_lib.content_hash, k, words)
        assert trials == 2_000
        if hits:
            bad[k] = hits
    assert not bad, bad


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rescalings_over_adjacent_words_never_collide(dtype):
    """rescalings that touch both halves of two adjacent words of one lane (float64: both words)"""
    hits, trials = chc.window_rescalings(_lib.content_hash, dtype)
    assert trials == 20_000 and hits == 0, (hits, trials)


def test_swaps_change_the_hash():
    """(d) two words of one lane, two 32-byte groups, two whole 1 MiB blocks"""
    rng = np.random.default_rng(21)
    base = chc.seeded_bytes(64 * 8, seed=22).view(np.uint64)
    h0 = _lib.content_hash(base)
    for _ in range(500):
        lane = int(rng.integers(4))
        i, j = (lane + 4 * rng.choice(16, 2, replace=False)).tolist()
        a = base.copy()
        a[[i, j]] = a[[j, i]]
        assert a.tobytes() != base.tobytes() and _lib.content_hash(a) != h0, (i, j)
    groups = base.reshape(16, 4)
    for i in range(16):
        for j in range(i + 1, 16):
            a = groups.copy()
            a[[i, j]] = a[[j, i]]
            assert a.tobytes() != base.tobytes() and _lib.content_hash(a) != h0, (i, j)
    big = chc.seeded_bytes(3 * chc.BLOCK + 5, seed=23)
    hb = _lib.content_hash(big)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        a = big.copy()
        a[i * chc.BLOCK:(i + 1) * chc.BLOCK] = big[j * chc.BLOCK:(j + 1) * chc.BLOCK]
        a[j * chc.BLOCK:(j + 1) * chc.BLOCK] = big[i * chc.BLOCK:(i + 1) * chc.BLOCK]
        assert a.tobytes() != big.tobytes() and _lib.content_hash(a) != hb, (i, j)
    # a block of equal content at another place: two blocks of the same bytes, then only the block index tells them apart
    twin = np.concatenate([big[:chc.BLOCK], big[:chc.BLOCK], big[chc.BLOCK:2 * chc.BLOCK]])
    other = np.concatenate([big[:chc.BLOCK], big[chc.BLOCK:2 * chc.BLOCK], big[:chc.BLOCK]])
    assert _lib.content_hash(twin) != _lib.content_hash(other)


@pytest.mark.parametrize("tail", [2, 7, 8, 9, 31])
def test_an_edit_moved_within_and_out_of_the_ragged_tail(tail):
    """(e) the last < 32 bytes go to lane 0 byte by byte: the same xor at another byte of the tail, or at a byte of the last whole group
    instead, is another buffer"""
    for groups in (0, 1, 5):
        n = 32 * groups + tail
        base = chc.seeded_bytes(n, seed=31 + tail)
        seen = {_lib.content_hash(base): "base"}
        for at in list(range(max(0, n - tail - 32), n)):
            for v in (1, 0x80, 0xFF):
                a = base.copy()
                a[at] ^= v
                h = _lib.content_hash(a)
                assert h not in seen, (n, at, v, seen[h])
                seen[h] = (at, v)
        assert len(seen) == 1 + 3 * min(n, tail + 32)


def test_zeros_appended_change_the_hash():
    """(f) the length is in the result, and a zero byte or word is absorbed like any other"""
    base = chc.seeded_bytes(chc.BLOCK - 16, seed=41)
    seen = set()
    for extra in [0, 1, 2, 7, 8, 15, 16, 17, 31, 32, 33, 48, 64, chc.BLOCK, chc.BLOCK + 16]:
        seen.add(_lib.content_hash(np.concatenate([base, np.zeros(extra, np.uint8)])))
        seen.add(_lib.content_hash(np.concatenate([base[:40], np.zeros(extra, np.uint8)])))
        seen.add(_lib.content_hash(np.zeros(extra, np.uint8)))
    assert len(seen) == 3 * 15


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
def test_one_hot_entry_moved(dtype):
    """(g) 20 000 drawn positions of the only non-zero entry: one hash per position, none equal to the all-zero buffer's"""
    hashes, positions = chc.one_hot_moves(_lib.content_hash, dtype)
    assert positions > 10_000 and hashes == positions, (hashes, positions)


@pytest.fixture(scope="module")
def big_scipy():
    """the construction of test_adjacency_fingerprint_hashes_every_entry (tests/test_host_cpu.py)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(0)
    n, nnz = 4000, 900_000
    return sp.csr_matrix((rng.random(nnz).astype(np.float32), (rng.integers(0, n, nnz), rng.integers(0, n, nnz))), shape=(n, n))


SAME_LANE = {np.float32: [(1, 9), (3, 8003), (800_001, 800_009),       # odd float32 indices, 8 k apart: one lane, sign in bit 63
                          (1, 8, 9), (8, 9, 17), (800_001, 800_008, 800_009)],     # and with both halves of the lane's next word
             np.float64: [(1, 5), (2, 4002), (800_001, 800_005), (1, 5, 9)]}      # float64 indices 4 k apart


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_paired_negation_through_the_callers(big_scipy, dtype):
    """two or three same-lane entries of m.data negated in place: AdjIdentity stops matching (and matches again when the edit is undone),
    hopcache.content_key of the array and of a CPU tensor over it changes"""
    from sgl_amd.hopcache import content_key
    from sgl_amd.operators.base_op import AdjIdentity
    m = big_scipy.astype(dtype)
    assert m.data.dtype == dtype and m.nnz > 850_000
    ident = AdjIdentity(m)
    assert ident.matches(m)
    for at in SAME_LANE[dtype]:
        at = list(at)
        assert len({chc.lane_of(dtype, i) for i in at}) == 1 and (m.data[at] != 0).all()
        assert len({(i * m.data.itemsize) // chc.BLOCK for i in at}) == 1                         # one 1 MiB block, too
        key_m, key_a, key_t = content_key(m), content_key(m.data), content_key(torch.from_numpy(m.data))
        m.data[at] *= -1
        assert not ident.matches(m), at
        assert content_key(m) != key_m and content_key(m.data) != key_a and content_key(torch.from_numpy(m.data)) != key_t, at
        m.data[at] *= -1
        assert ident.matches(m) and content_key(m) == key_m and content_key(m.data) == key_a
