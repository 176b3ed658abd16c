"""Shared by the tests of sgl_content_hash (tests/test_content_hash_cpu.py, tests/test_gpu_host_shims.py): a serial restatement of the
function from the text at its declaration in include/sgl_hip.h, and the families of edits that a content key must tell apart.

A "lane" is what the header says: the 64-bit words of a block are dealt to four lanes in turn, so words k and k + 4 share a lane,
float64 elements i and i + 4 do, float32 / int32 elements i and j do when (i // 2) % 4 == (j // 2) % 4."""
import numpy as np

MASK = (1 << 64) - 1
BLOCK = 1 << 20
GROUP = 32
M1, M2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
LANE_SEEDS = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x27D4EB2F165667C5)
FOLD_SEED, TOTAL_SEED = 0x2545F4914F6CDD1D, 0xCBF29CE484222325


def step(h, v):
    t = (h ^ v) * M1                      # the full 128-bit product
    return (t & MASK) ^ (t >> 64)


def fmix(h):
    h = ((h ^ (h >> 30)) * M1) & MASK
    h = ((h ^ (h >> 27)) * M2) & MASK
    return h ^ (h >> 31)


def block_part(b, raw):
    """part[b] of the header text for the bytes `raw` of block b"""
    h = [LANE_SEEDS[0] ^ b, LANE_SEEDS[1], LANE_SEEDS[2], LANE_SEEDS[3]]
    groups = len(raw) // GROUP
    words = np.frombuffer(raw[:groups * GROUP], dtype=np.uint64).reshape(groups, 4)      # host byte order, as memcpy loads them
    for k in range(4):
        hk = h[k]
        for w in words[:, k].tolist():
            hk = step(hk, w)
        h[k] = hk
    for byte in raw[groups * GROUP:]:
        h[0] = step(h[0], byte)
    e = FOLD_SEED
    for hk in h:
        e = step(e, hk)
    return fmix(e)


def serial_hash(buf):
    """sgl_content_hash of the bytes of `buf` (anything np.asarray takes, C-contiguous), one thread, block after block"""
    raw = np.ascontiguousarray(buf).view(np.uint8).reshape(-1).tobytes()
    h = TOTAL_SEED ^ len(raw)
    for b in range((len(raw) + BLOCK - 1) // BLOCK):
        h = step(h, block_part(b, raw[b * BLOCK:(b + 1) * BLOCK]))
    return fmix(h)


LENGTHS = [0, 1, 7, 8, 31, 32, 33, 63, 64, BLOCK - 1, BLOCK, BLOCK + 1, BLOCK + 32, 3 * BLOCK + 5]


def seeded_bytes(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


def seeded_values(dtype, count, seed):
    """ordinary data of `dtype`: normal floats (no zeros, no NaN: every edit below changes the bytes) or full-range integers"""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "f":
        v = rng.standard_normal(count).astype(dtype)
        v[v == 0] = 1
        return v
    return rng.integers(-2 ** 31, 2 ** 31 - 1, count, dtype=np.int64).astype(dtype)


def lane_of(dtype, i):
    return (i * np.dtype(dtype).itemsize // 8) % 4


def same_lane_pairs(dtype, count):
    """every pair i < j of element positions of a `count`-element buffer whose 64-bit words share a lane (of block 0)"""
    return [(i, j) for i in range(count) for j in range(i + 1, count) if lane_of(dtype, i) == lane_of(dtype, j)]


def flip_sign(a, i):
    """negate element i in place by its top bit (floats: exactly -x; int32: the top bit of the word)"""
    bits = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    bits[i] ^= bits.dtype.type(1) << bits.dtype.type(8 * a.dtype.itemsize - 1)


def count_collisions(hash_fn, base, edits):
    """`edits` yields functions that edit a copy of `base` in place; -> (collisions with the hash of `base`, trials).  An edit that
    leaves the bytes as they were is an error of the test, not a trial."""
    h0 = hash_fn(base)
    raw0 = base.tobytes()
    hits = trials = 0
    for edit in edits:
        a = base.copy()
        edit(a)
        assert a.tobytes() != raw0, "the edit did not change the bytes"
        trials += 1
        hits += hash_fn(a) == h0
    return hits, trials


def paired_sign_flips(hash_fn, dtype, count=64, seed=11):
    """family (a), exhaustive over a `count`-element buffer"""
    base = seeded_values(dtype, count, seed)

    def edits():
        for i, j in same_lane_pairs(dtype, count):
            def edit(a, i=i, j=j):
                flip_sign(a, i)
                flip_sign(a, j)
            yield edit
    return count_collisions(hash_fn, base, edits())


def paired_rescalings(hash_fn, dtype, trials=20_000, count=256, seed=12):
    """family (b): two same-lane values each multiplied by 2^k, k in [-6, 6] without 0.  Of a 4-byte type only the elements in the
    upper half of their word are drawn (odd indices): their exponent bits are the top bits of the word, the sharpest case"""
    base = seeded_values(dtype, count, seed)
    rng = np.random.default_rng(seed + 1)
    pairs = [(i, j) for i, j in same_lane_pairs(dtype, count) if np.dtype(dtype).itemsize == 8 or (i % 2 and j % 2)]
    ks = np.array([k for k in range(-6, 7) if k != 0])

    def edits():
        for _ in range(trials):
            i, j = pairs[rng.integers(len(pairs))]
            ki, kj = rng.choice(ks, 2)

            def edit(a, i=i, j=j, ki=ki, kj=kj):
                a[i] = np.ldexp(a[i], ki)
                a[j] = np.ldexp(a[j], kj)
            yield edit
    return count_collisions(hash_fn, base, edits())


def top_bit_masks(hash_fn, k, words, trials=2_000, count=128, seed=13):
    """family (c): non-zero xor masks confined to the top k bits of `words` 64-bit words of one lane"""
    base = seeded_bytes(count * 8, seed + k).view(np.uint64)
    rng = np.random.default_rng(seed + 100 * words + k)

    def edits():
        for _ in range(trials):
            lane = int(rng.integers(4))
            at = lane + 4 * rng.choice(count // 4, words, replace=False)
            masks = rng.integers(1, 1 << k, words, dtype=np.uint64) << np.uint64(64 - k)

            def edit(a, at=at, masks=masks):
                a[at] ^= masks
            yield edit
    return count_collisions(hash_fn, base, edits())


def one_hot_moves(hash_fn, dtype, trials=20_000, count=1 << 15, seed=14):
    """family (g): -> (distinct hashes, distinct positions) of a one-hot buffer whose entry sits at `trials` drawn positions, the
    all-zero buffer counted as one more position"""
    rng = np.random.default_rng(seed)
    a = np.zeros(count, dtype)
    hashes, positions = {hash_fn(a)}, {-1}
    for p in rng.integers(0, count, trials).tolist():
        a[p] = 1
        hashes.add(hash_fn(a))
        positions.add(p)
        a[p] = 0
    return len(hashes), len(positions)


# ---- small windows of one lane: the edits that a step with a FIXED low-weight state difference lets cancel ---------------------------
def window_elements(dtype, first_word, words):
    """the element positions of `words` consecutive words of one lane: 64-bit words first_word, first_word + 4, ..."""
    per = 8 // np.dtype(dtype).itemsize
    return [w * per + e for w in range(first_word, first_word + 4 * words, 4) for e in range(per)]


def windows(dtype, words, buffers, seed, count_words=48):
    """`buffers` seeded buffers of count_words 64-bit words, each with a window of `words` consecutive same-lane words: drawn, and
    for every other buffer the lane's LAST words (the difference then meets the fold of the lanes, not a further word)"""
    per = 8 // np.dtype(dtype).itemsize
    rng = np.random.default_rng(seed)
    for b in range(buffers):
        last = count_words - 4 * (words - 1) - 1
        first = last - int(rng.integers(4)) if b % 2 else int(rng.integers(0, last + 1))
        yield seeded_values(dtype, count_words * per, seed + 1000 + b), window_elements(dtype, first, words)


def window_sign_flips(hash_fn, dtype, words, buffers=40, seed=15):
    """EVERY non-empty subset of sign flips over the elements of `words` consecutive same-lane words (both halves of a word of a 4-byte
    type), for each of `buffers` windows; -> (collisions, trials)"""
    hits = trials = 0
    for base, at in windows(dtype, words, buffers, seed):
        def edits(at=at):
            for subset in range(1, 1 << len(at)):
                def edit(a, subset=subset):
                    for q, i in enumerate(at):
                        if subset >> q & 1:
                            flip_sign(a, i)
                yield edit
        h, t = count_collisions(hash_fn, base, edits())
        hits, trials = hits + h, trials + t
    return hits, trials


def both_half_masks(hash_fn, k, words, trials=2_000, count=128, seed=16):
    """xor masks confined to the top k bits of BOTH 32-bit halves (bits 63 .. 64 - k and 31 .. 32 - k) of `words` words of one lane,
    consecutive in the lane in every other trial; no word's mask is zero"""
    base = seeded_bytes(count * 8, seed + k).view(np.uint64)
    rng = np.random.default_rng(seed + 100 * words + k)

    def edits():
        for trial in range(trials):
            lane = int(rng.integers(4))
            if trial % 2:
                at = lane + 4 * (int(rng.integers(0, count // 4 - words + 1)) + np.arange(words))
            else:
                at = lane + 4 * rng.choice(count // 4, words, replace=False)
            both = rng.integers(1, 1 << 2 * k, words, dtype=np.uint64)                     # 2 k bits, not all zero
            masks = ((both >> np.uint64(k)) << np.uint64(64 - k)) | ((both & np.uint64((1 << k) - 1)) << np.uint64(32 - k))

            def edit(a, at=at, masks=masks):
                a[at] ^= masks
            yield edit
    return count_collisions(hash_fn, base, edits())


def window_rescalings(hash_fn, dtype, trials=20_000, count_words=64, seed=17):
    """two ADJACENT words of one lane: of a 4-byte type a drawn subset of their four elements that holds an element of the upper and one
    of the lower half, of float64 both words; each chosen element times 2^k, k in [-6, 6] without 0"""
    per = 8 // np.dtype(dtype).itemsize
    base = seeded_values(dtype, count_words * per, seed)
    rng = np.random.default_rng(seed + 1)
    ks = np.array([k for k in range(-6, 7) if k != 0])
    subsets = [s for s in range(1, 1 << 2 * per) if per == 1 and s == 3 or per == 2 and s & 0b0101 and s & 0b1010]

    def edits():
        for _ in range(trials):
            at = window_elements(dtype, int(rng.integers(0, count_words - 4)), 2)
            subset = subsets[rng.integers(len(subsets))]
            chosen = [i for q, i in enumerate(at) if subset >> q & 1]
            scale = rng.choice(ks, len(chosen))

            def edit(a, chosen=chosen, scale=scale):
                for i, k in zip(chosen, scale):
                    a[i] = np.ldexp(a[i], k)
            yield edit
    return count_collisions(hash_fn, base, edits())
