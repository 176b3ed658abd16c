"""What the CSR-merge tests share (csrc/sgl_csr_merge.hip, device.csr_merge, sgl_amd/transforms.py add_edges / add_self_loops /
to_undirected): a vectorised numpy reference of the merge that include/sgl_hip.h states -- keys row * n_cols + col, both modes, both
position arrays -- the plain per-row two-pointer loop it is proven equal to, a numpy emulation of the kernel's slot rule (and of two
wrong ones), and the zoo of small matrix pairs the kernels are run on.

A matrix is a scipy csr_matrix built from its three arrays, never canonicalised: the bits of the values stay as they are."""
import numpy as np
import scipy.sparse as sp

LANES = (4, 16, 64)
SUM, KEEP = 0, 1
MODES = {"sum": SUM, "keep": KEEP}
F = np.float32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def keys(m):
    indptr = np.asarray(m.indptr, dtype=np.int64)
    rows = np.repeat(np.arange(m.shape[0], dtype=np.int64), np.diff(indptr))
    return rows * np.int64(max(m.shape[1], 1)) + np.asarray(m.indices, dtype=np.int64)


def merge_reference(a, b, mode=SUM):
    """(indptr int64, indices int32, data float32, pos_a int64, pos_b int64) of the union of the canonical CSRs a and b"""
    assert a.shape == b.shape
    n_rows, n_cols = a.shape
    ka, kb = keys(a), keys(b)
    assert np.all(np.diff(ka) > 0) and np.all(np.diff(kb) > 0), "canonical inputs: sorted and unique"
    union = np.union1d(ka, kb)

    def where(k):
        p = np.searchsorted(k, union)
        hit = p < len(k)
        hit[hit] = k[p[hit]] == union[hit]
        return np.where(hit, p, -1).astype(np.int64)

    pa, pb = where(ka), where(kb)
    av, bv = np.asarray(a.data, dtype=F), np.asarray(b.data, dtype=F)
    bits = np.zeros(len(union), dtype=np.uint32)
    only_a, only_b, both = (pa >= 0) & (pb < 0), (pa < 0) & (pb >= 0), (pa >= 0) & (pb >= 0)
    bits[only_a] = av.view(np.uint32)[pa[only_a]]
    bits[only_b] = bv.view(np.uint32)[pb[only_b]]
    with np.errstate(all="ignore"):
        summed = (av[pa[both]] + bv[pb[both]]).astype(F) if mode == SUM else av[pa[both]]
    bits[both] = summed.view(np.uint32)
    indptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(union // max(n_cols, 1), minlength=n_rows)[:n_rows], out=indptr[1:])
    return indptr, (union % max(n_cols, 1)).astype(np.int32), bits.view(F), pa, pb


def merge_loop(a, b, mode=SUM):
    """the same by a plain two-pointer walk of every row"""
    indptr, cols, bits, pa, pb = [0], [], [], [], []
    ab, bb = np.asarray(a.data, dtype=F), np.asarray(b.data, dtype=F)
    for i in range(a.shape[0]):
        p, pe, q, qe = int(a.indptr[i]), int(a.indptr[i + 1]), int(b.indptr[i]), int(b.indptr[i + 1])
        while p < pe or q < qe:
            ca = a.indices[p] if p < pe else None
            cb = b.indices[q] if q < qe else None
            if cb is None or (ca is not None and ca < cb):
                cols.append(ca), bits.append(ab[p:p + 1].view(np.uint32)[0]), pa.append(p), pb.append(-1)
                p += 1
            elif ca is None or cb < ca:
                cols.append(cb), bits.append(bb[q:q + 1].view(np.uint32)[0]), pa.append(-1), pb.append(q)
                q += 1
            else:
                with np.errstate(all="ignore"):
                    v = F(ab[p] + bb[q]) if mode == SUM else ab[p]
                cols.append(ca), bits.append(np.array([v], dtype=F).view(np.uint32)[0]), pa.append(p), pb.append(q)
                p, q = p + 1, q + 1
        indptr.append(len(cols))
    return (np.array(indptr, dtype=np.int64), np.array(cols, dtype=np.int32), np.array(bits, dtype=np.uint32).view(F),
            np.array(pa, dtype=np.int64), np.array(pb, dtype=np.int64))


def as_matrix(result, shape):
    indptr, indices, data = result[:3]
    return sp.csr_matrix((data, indices, indptr), shape=shape)


def scipy_concatenated(a, b):
    """the reference's way: csr_matrix((w, (row, col))) of the two COO lists one after the other"""
    ra = np.repeat(np.arange(a.shape[0]), np.diff(a.indptr))
    rb = np.repeat(np.arange(b.shape[0]), np.diff(b.indptr))
    m = sp.csr_matrix((np.concatenate((a.data, b.data)).astype(F), (np.concatenate((ra, rb)), np.concatenate((a.indices, b.indices)))),
                      shape=a.shape)
    m.sum_duplicates()
    m.sort_indices()
    return m


def agrees(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_bits(got[2], want[2])
            and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4]))


SENTINEL = -77


def slot_fill(a, b, indptr, rule="right"):
    """The kernel's slot rule in numpy, entry by entry, on a sentinel-filled output row guarded like the kernel's: (indices, pos_a,
    pos_b).  A's k-th entry goes to k + lower_bound_B(column) - (common columns before it); a B entry that A stores writes nothing;
    the others go to (their rank among B's own) + lower_bound_A(column).
    rule "no_common": the common count is not subtracted on either side; "upper": the bound is taken as the upper bound."""
    side = "right" if rule == "upper" else "left"
    total = int(indptr[-1])
    cols = np.full(total, SENTINEL, dtype=np.int32)
    pa, pb = np.full(total, SENTINEL, dtype=np.int64), np.full(total, SENTINEL, dtype=np.int64)
    for i in range(a.shape[0]):
        a0, a1, b0, b1 = int(a.indptr[i]), int(a.indptr[i + 1]), int(b.indptr[i]), int(b.indptr[i + 1])
        ac, bc = np.asarray(a.indices[a0:a1]), np.asarray(b.indices[b0:b1])
        out, out_end = int(indptr[i]), int(indptr[i + 1])
        in_b, in_a = np.isin(ac, bc), np.isin(bc, ac)
        common_before = np.cumsum(in_b) - in_b
        slots = np.arange(len(ac)) + np.searchsorted(bc, ac, side=side) - (0 if rule == "no_common" else common_before)
        where_b = np.searchsorted(bc, ac)
        for k, o in enumerate(out + slots):
            if out <= o < out_end:
                cols[o], pa[o], pb[o] = ac[k], a0 + k, (b0 + where_b[k] if in_b[k] else -1)
        rank = np.arange(len(bc)) if rule == "no_common" else np.cumsum(~in_a) - (~in_a)
        slots = rank + np.searchsorted(ac, bc, side=side)
        for k, o in enumerate(out + slots):
            if not in_a[k] and out <= o < out_end:
                cols[o], pa[o], pb[o] = bc[k], -1, b0 + k
    return cols, pa, pb


def common_followed(a, b):
    """does some row hold a common column that is not the last column of the row's union?"""
    want = merge_reference(a, b)
    both = (want[3] >= 0) & (want[4] >= 0)
    last = np.zeros(len(both), dtype=bool)
    ends = want[0][1:][np.diff(want[0]) > 0] - 1
    last[ends] = True
    return bool((both & ~last).any())


# ---- the zoo ---------------------------------------------------------------------------------------------------------------------------
ZOO_LENGTHS = (3, 4, 5, 15, 16, 17, 63, 64, 65, 129, 257)
BOUNDARIES = (3, 4, 15, 16, 63, 64, 127, 128, 255, 256)       # the positions on both sides of every stride boundary of every G
SPECIAL_A = np.array([0x80000000, 0x7FC01234, 0x7F800000, 0x00000001, 0x00000000, 0xFF800000, 0xFFC0ABCD, 0x807FFFFF], dtype=np.uint32)
SPECIAL_B = np.array([0x00000000, 0x3FC00000, 0x7F800000, 0x00000001, 0x80000000, 0xFF800000, 0x40000000, 0x00000002], dtype=np.uint32)
#             sums:   -0 + 0 = +0, NaN(payload) + 1.5 = that NaN, inf + inf, denormal + denormal, 0 + -0 = +0, -inf + -inf, NaN + 2, denormals
# never NaN + NaN and never inf - inf: which NaN comes out of those is the adder's choice, not the contract's


def _build(n_cols, rows_a, rows_b, rng, specials=()):
    """rows_*: a list of sorted column arrays.  Values: finite random float32, except rows listed in `specials` (same length on both
    sides): the special bit patterns above, in order"""
    def one(rows, special):
        indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
        indices = (np.concatenate(rows) if indptr[-1] else np.zeros(0)).astype(np.int32)
        data = ((rng.rand(len(indices)) - 0.5) * 8).astype(F)
        for i in specials:
            k = min(len(rows[i]), len(special))
            data[indptr[i]:indptr[i] + k] = special[:k].view(F)
        return sp.csr_matrix((data, indices, indptr), shape=(len(rows), n_cols))
    a, b = one(rows_a, SPECIAL_A), one(rows_b, SPECIAL_B)
    for m in (a, b):
        assert all(np.all(np.diff(m.indices[m.indptr[i]:m.indptr[i + 1]]) > 0) for i in range(m.shape[0]))
    return a, b


def _forced(la, lb, n_cols, rng):
    """(A's columns, B's columns): B random, A holds B's columns at the boundary positions and random others -- la and lb exactly"""
    universe = rng.permutation(min(n_cols, 2 * (la + lb)))
    bc = np.sort(universe[:lb])
    forced = bc[[k for k in BOUNDARIES if k < lb]][:la]
    rest = np.setdiff1d(universe, forced)
    ac = np.sort(np.concatenate((forced, rng.permutation(rest)[:la - len(forced)])))
    assert len(ac) == la and len(bc) == lb
    return ac, bc


def zoo():
    """name -> (a, b): every pair small (n <= 300 rows, the longest row about 3 000 entries)"""
    rng = np.random.RandomState(15)
    out = {}
    n_cols = 7001
    ar = np.arange
    ra, rb, special = [], [], []

    def add(x, y, is_special=False):
        if is_special:
            special.append(len(ra))
        ra.append(np.asarray(x, dtype=np.int64)), rb.append(np.asarray(y, dtype=np.int64))

    add([], [])                                                      # empty on both sides, first row
    add([], [5, 9, 7000])
    add([0, 3, 6999], [])
    add([2, 40, 41, 300, 6000, 6001, 6002, 7000], [2, 40, 41, 300, 6000, 6001, 6002, 7000], True)      # identical, the special values summed
    add(ar(64) * 3, ar(64) * 3)                                      # identical, one whole wavefront
    add(ar(17) * 2, ar(17) * 2 + 1)                                  # disjoint, interleaved
    add(ar(8) * 2 + 100, ar(8) * 2 + 101, True)                      # disjoint, the special values copied
    add(ar(20) + 500, ar(20))                                        # B wholly before A
    add(ar(20), ar(20) + 500)                                        # B wholly after A
    add(ar(70), ar(70) + 70)
    add([10, 20, 30, 40, 50], [10, 60, 70])                          # a single common column at the first position
    add([10, 20, 30, 40, 50], [1, 2, 50])                            # ... at the last position
    add([10, 20], [10])
    add([10], [5, 10])
    add([33], [33])
    for la in ZOO_LENGTHS:
        for lb in ZOO_LENGTHS:
            x, y = _forced(la, lb, n_cols, rng)
            add(x, y)                                                # common columns around the stride boundaries of B's walk
            y, x = _forced(lb, la, n_cols, rng)
            add(x, y)                                                # ... of A's walk
    hub = np.sort(rng.permutation(n_cols)[:3001])
    add(hub, [int(hub[1500])])                                       # a hub against a row of one (common)
    add([int(hub[7])], hub)
    add(hub[:3000], np.sort(np.concatenate((hub[:3000:2], np.setdiff1d(ar(n_cols), hub)[:1500]))))   # every second column common
    add([], [])                                                      # the last row is empty
    assert len(ra) <= 300
    out["main"] = _build(n_cols, ra, rb, rng, specials=special)
    out["one_row"] = _build(400, [np.sort(rng.permutation(400)[:100])], [np.sort(rng.permutation(400)[:80])], rng)
    some = [np.sort(rng.permutation(9)[:k]) for k in (0, 3, 9, 1, 4)]
    none = [np.zeros(0, dtype=np.int64)] * 5
    out["a_empty"] = _build(9, none, some, rng)
    out["b_empty"] = _build(9, some, none, rng)
    out["both_empty"] = _build(9, none, none, rng)
    out["square"] = _build(37, [np.sort(rng.permutation(37)[:rng.randint(0, 20)]) for _ in range(37)],
                           [np.sort(rng.permutation(37)[:rng.randint(0, 20)]) for _ in range(37)], rng)
    out["tall"] = _build(11, [np.sort(rng.permutation(11)[:rng.randint(0, 12)]) for _ in range(203)],
                         [np.sort(rng.permutation(11)[:rng.randint(0, 12)]) for _ in range(203)], rng)
    a, b = out["square"]                                             # cancellation: b = -a on every common column of the first rows
    ka, kb = keys(a), keys(b)
    hit = np.nonzero(np.isin(kb, ka))[0][:10]
    b.data[hit] = -a.data[np.searchsorted(ka, kb[hit])]
    return out


_ZOO = None


def shared_zoo():
    global _ZOO
    if _ZOO is None:
        _ZOO = zoo()
    return _ZOO


# ---- G22 -------------------------------------------------------------------------------------------------------------------------------
G22_GRAPHS = ("sym64", "pl256", "dir40", "symdiag48")


def canonical(m):
    m = sp.csr_matrix(m)
    m.sum_duplicates()
    m.sort_indices()
    return m


def recorded(goldens, key):
    g = goldens.npz("g22_merge_transforms")
    return sp.csr_matrix((g[key + "|data"], g[key + "|indices"], g[key + "|indptr"]), shape=tuple(g[key + "|shape"]))


def g22_graph(goldens, name):
    return recorded(goldens, name) if name == "symdiag48" else canonical(goldens.graph(name).astype(F))


def storage_order_csr(idx, w, shape):
    """The ingest's contract for the added list (sgl_ingest.hip): a canonical CSR in which a repeated pair holds the float32 sum of
    its weights in storage order"""
    idx, w = np.asarray(idx, dtype=np.int64), np.asarray(w, dtype=F)
    key = idx[0] * shape[1] + idx[1]
    order = np.argsort(key, kind="stable")
    uniq, first = np.unique(key[order], return_index=True)
    data = np.zeros(len(uniq), dtype=F)
    ends = np.concatenate((first[1:], [len(key)]))
    for k, (s, e) in enumerate(zip(first, ends)):
        acc = w[order[s]]
        for t in order[s + 1:e]:
            acc = F(acc + w[t])
        data[k] = acc
    indptr = np.zeros(shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(uniq // shape[1], minlength=shape[0]), out=indptr[1:])
    return sp.csr_matrix((data, (uniq % shape[1]).astype(np.int32), indptr), shape=shape)


def multiplicity(a, idx):
    """per entry of the union of `a` and the added list: how often the pair occurs in the concatenation (keys ascending)"""
    key = np.concatenate((keys(a), np.asarray(idx[0], dtype=np.int64) * a.shape[1] + np.asarray(idx[1], dtype=np.int64)))
    return np.unique(key, return_counts=True)


def check_against_add_golden(got, a, idx, w, golden):
    """`got` (a canonical scipy CSR) against the reference's add_edges(...).sparse_matrix under the stated condition: the structure
    is the golden's; every pair that occurs at most twice in the concatenation is bit-equal to the golden; exactly ONE pair occurs
    three times, there `got` holds a + (b1 + b2) -- the model -- and the golden holds something else."""
    model = as_matrix(merge_reference(a, storage_order_csr(idx, w, a.shape), SUM), a.shape)
    assert np.array_equal(got.indptr, golden.indptr) and np.array_equal(got.indices, golden.indices)
    key, count = multiplicity(a, idx)
    assert np.array_equal(key, keys(golden)) and count.max() == 3 and (count == 3).sum() == 1
    few = count <= 2
    assert same_bits(got.data[few].astype(F), golden.data[few].astype(F))
    assert same_bits(got.data.astype(F), model.data.astype(F))
    assert not same_bits(model.data[~few].astype(F), golden.data[~few].astype(F))


def check_against_del_golden(got, a, idx, w, golden):
    """add_edges(del_repeated=True).  The reference keeps whichever duplicate its unstable argsort puts first, so where a pair occurs
    more than once its recorded value is ONE of the candidates; here the stored value always wins and the duplicates of the added
    list stand as their storage-order sum (the documented difference).  Structure: exact.  Pairs that occur once: bit-equal."""
    added = storage_order_csr(idx, w, a.shape)
    model = as_matrix(merge_reference(a, added, KEEP), a.shape)
    assert np.array_equal(got.indptr, golden.indptr) and np.array_equal(got.indices, golden.indices)
    assert same_bits(got.data.astype(F), model.data.astype(F))
    key, count = multiplicity(a, idx)
    once = count == 1
    assert same_bits(got.data[once].astype(F), golden.data[once].astype(F)) and once.sum() > 10
    ka = keys(a)
    lk = np.asarray(idx[0], dtype=np.int64) * a.shape[1] + np.asarray(idx[1], dtype=np.int64)
    for k, v in zip(key[~once], golden.data[~once]):
        cands = list(np.asarray(w, dtype=F)[lk == k]) + list(a.data[ka == k])
        assert any(same_bits(np.array([v], dtype=F), np.array([c], dtype=F)) for c in cands), (k, v, cands)
