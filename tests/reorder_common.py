"""What the reorder tests share (csrc/sgl_reorder.hip: sgl_reorder_community, sgl_reorder_lpa_round, sgl_csr_permute_rows): the per-node
rule of lpa_round_kernel in numpy, written from the kernel's header comment, the rows whose neighbour labels are laid out so that the
kernel's SAMPLE of a long row decides the answer, and the matrices of the row permutation.  Everything is integers: every comparison
is exact."""
import functools

import numpy as np
import scipy.sparse as sp

SAMPLE = 256
M64 = (1 << 64) - 1


def lpa_active(node, rnd, last):
    """may `node` move in round `rnd`?  A hash of node and round, computed in 64 bits with wrap-around; everybody in the last round"""
    if last:
        return True
    x = (int(node) ^ ((int(rnd) * 2654435761 + 12345) & M64)) & M64
    x = ((x * 0x9E3779B97F4A7C15) & M64) & 0x7FFFFFFFFFFFFFFF
    x = (x >> 29) ^ x
    return (x & 1) == (int(rnd) & 1)


def lpa_round_reference(rowptr, col, labels, rnd, last, row0=0, sample=SAMPLE):
    """One round for the rows [row0, row0 + n) of a matrix (rowptr local to the block, global column ids, labels of ALL nodes).
    A node without neighbours or an inactive one keeps its label.  Every other node looks at col[p0 + j * step], j < min(deg, sample),
    step = max(1, deg // sample), and adopts the most frequent label, ties to the smaller one.  sample=None: every neighbour.
    Returns (the block's new labels int32, how many of them changed)."""
    rowptr, col, labels = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(labels)
    n = len(rowptr) - 1
    out = np.empty(n, dtype=np.int32)
    moved = 0
    for i in range(n):
        mine = labels[row0 + i]
        p0, deg = int(rowptr[i]), int(rowptr[i + 1] - rowptr[i])
        if deg == 0 or not lpa_active(row0 + i, rnd, last):
            out[i] = mine
            continue
        length, step = (deg, 1) if sample is None else (min(deg, sample), max(1, deg // sample))
        seen, count = np.unique(labels[col[p0 + step * np.arange(length)]], return_counts=True)
        out[i] = seen[np.argmax(count)]                               # `seen` ascends and argmax takes the first maximum: the smaller label
        moved += int(out[i] != mine)
    return out, moved


def community_order_from_rounds(rowptr, col, n, rounds=8, sample=SAMPLE):
    """`rounds` rounds from the identity labels, the last one with everybody active, then a stable sort of the nodes by label.
    Returns (order int64 with order[i] = position of node i, number of communities, nodes moved in the last round)."""
    labels = np.arange(n, dtype=np.int32)
    moved = 0
    for it in range(rounds):
        labels, moved = lpa_round_reference(rowptr, col, labels, it, it == rounds - 1, 0, sample)
    perm = np.argsort(labels, kind="stable")
    order = np.empty(n, dtype=np.int64)
    order[perm] = np.arange(n)
    return order, len(np.unique(labels)), moved


def info_text(n_comm, rounds, moved):
    return f"{n_comm} communities after {rounds} rounds, {moved} nodes moved in the last"


# ---- rows with constructed neighbour labels --------------------------------------------------------------------------------------------
def build_block(specs, row0=0, seed=0):
    """specs: one (own label, sequence of neighbour labels) per row of the block.  The block's rows are the nodes row0 ... ; every row
    gets a range of column ids of its own, ascending, behind the block's nodes, and the labels of those nodes are the sequence: a
    canonical CSR in which position j of row i has exactly the label asked for.  The nodes in front of the block get random labels.
    Returns dict(rowptr, col, labels, row0, n_local, n_global)."""
    n_local = len(specs)
    first = row0 + n_local
    deg = np.array([len(s[1]) for s in specs], dtype=np.int64)
    n_global = first + int(deg.sum())
    rowptr = np.concatenate(([0], np.cumsum(deg))).astype(np.int64)
    col = (first + np.arange(int(deg.sum()))).astype(np.int32)
    labels = np.empty(n_global, dtype=np.int32)
    labels[:row0] = np.random.default_rng(seed).integers(0, n_global, row0)
    labels[row0:first] = [s[0] for s in specs]
    if deg.sum():
        labels[first:] = np.concatenate([np.asarray(s[1], dtype=np.int32) for s in specs if len(s[1])])
    assert labels.min() >= 0 and labels.max() < n_global
    assert not np.array_equal(labels, np.arange(n_global))
    return dict(rowptr=rowptr, col=col, labels=labels, row0=row0, n_local=n_local, n_global=n_global)


A, B, C, D = 40, 30, 20, 10            # labels: A > B > C > D


def alternate(deg, period, first, rest):
    """`first` at the positions that are multiples of `period`, `rest` elsewhere"""
    return np.where(np.arange(deg) % period == 0, first, rest)


def sampled_rows():
    """(name, own label, neighbour labels) of rows above 256 neighbours in which the 256 sampled positions and the full count give
    DIFFERENT labels (test_reorder_cpu asserts it): an index, stride or length that is off by one reads another label"""
    rows = []
    rows.append(("deg257 last entry never sampled", 7, [A] * 128 + [B] * 128 + [A]))                       # sample: tie -> B; all: A
    rows.append(("deg511 B behind position 254", 7, [A] * 255 + [B] * 256))                                 # sample: 255 A, 1 B -> A; all: B
    rows.append(("deg512 A even, B odd", 7, alternate(512, 2, A, B)))                                       # sample: A; all: tie -> B
    odd = [A] * 127 + [B] * 128                                                                             # positions 1, 3, ... 509
    even = [A] * 128 + [B] * 128                                                                            # positions 0, 2, ... 510: the sample
    body = np.empty(511, dtype=np.int64)
    body[0::2], body[1::2] = even, odd
    rows.append(("deg513 last two never sampled", 7, list(body) + [A, A]))                                  # sample: tie -> B; all: A by one
    rows.append(("deg768 every third", 7, alternate(768, 3, A, B)))                                         # sample: A; all: B
    seq = np.full(1000, B)
    seq[0:766:3] = A                                                                                        # step 3: positions 0 ... 765
    rows.append(("deg1000 every third of the first 766", 7, seq))                                           # sample: A; all: B
    return rows


def short_rows():
    """rows of at most 256 neighbours (nothing is sampled away) and the ties"""
    rng = np.random.default_rng(17)
    rows = [("deg1", 7, [A]),
            ("empty row between full ones", 9, []),
            ("deg64", 7, rng.choice([A, B, C], 64)),
            ("deg65 the 65th decides", 7, [A] * 32 + [B] * 32 + [A]),
            ("deg255", 7, rng.choice([A, B, C, D], 255)),
            ("deg256 tie of two", 7, alternate(256, 2, A, B)),
            ("deg511 as in the layout A 0-255, B 256-510", 7, [A] * 256 + [B] * 255),                       # sample and full count agree here
            ("tie of two, node moves", 9, [A, B, A, B]),
            ("tie of two, own label the larger: moves", A, [A, B, A, B]),
            ("tie of two, own label the smaller: stays", B, [A, B, A, B]),
            ("tie of four", C, [A, C, B, D] * 5),
            ("tie of four, own label the smallest", D, [D, A, C, B] * 5),
            ("tie across slots 64 apart", 7, [A] * 64 + [B] * 64),                                          # positions j and j + 64: lab[0] and lab[1] of a lane
            ("tie across three slots", 7, [B] * 64 + [A] * 64 + [C] * 64),
            ("tie across four slots", A, [B] * 64 + [A] * 64 + [D] * 64 + [C] * 64),
            ("one label per position", 7, 100 + np.arange(200)),                                            # 200 labels once each: the smallest
            ("majority in the last slot", 7, list(100 + np.arange(192)) + [A] * 2 + list(400 + np.arange(62)))]
    return rows


def filler_rows(count, seed):
    """rows of 0 ... 70 neighbours drawn from a few labels: ties are frequent"""
    rng = np.random.default_rng(seed)
    return [(f"filler {k}", int(rng.choice([A, B, C, D, 7])), rng.choice([A, B, C, D], int(rng.integers(0, 71)))) for k in range(count)]


@functools.lru_cache(maxsize=None)
def block_case(name, row0):
    if name == "sampled":
        rows = sampled_rows()
    elif name == "short":
        rows = short_rows()
    elif name.startswith("n"):                                        # n1 ... n5: the first rows of a list with an empty row inside; n1023: everything
        n = int(name[1:])
        rows = [short_rows()[k] for k in (2, 1, 3, 7, 5)][:n] if n <= 5 else (sampled_rows() + short_rows() + filler_rows(n, 23))[:n]
        assert len(rows) == n
    else:
        raise KeyError(name)
    blk = build_block([(own, seq) for _, own, seq in rows], row0=row0, seed=len(rows))
    blk["names"] = [r[0] for r in rows]
    return blk


BLOCK_CASES = ("sampled", "short", "n1", "n2", "n3", "n4", "n5", "n1023")
ROW0S = (0, 37)
ROUNDS = ((0, 0), (1, 0), (63, 0), (5, 1))                            # (round, last)


# ---- graphs ----------------------------------------------------------------------------------------------------------------------------
def planted_graph(n=3000, bs=100, hubs=3, hub_deg=900, seed=5):
    """planted communities of `bs` nodes behind shuffled ids, symmetric, with self-loops, and `hubs` rows far above 256 neighbours:
    the generator of test_gpu_parity's round-by-round test at a smaller size"""
    rng = np.random.default_rng(seed)
    a = np.repeat(np.arange(n), 10)
    near = np.minimum((a // bs) * bs + rng.integers(0, bs, a.size), n - 1)
    b = np.where(rng.random(a.size) < 0.85, near, rng.integers(0, n, a.size))
    if hubs:
        h = rng.choice(n, hubs, replace=False)
        a = np.concatenate([a, np.repeat(h, hub_deg)])
        b = np.concatenate([b, rng.integers(0, n, hubs * hub_deg)])
    m = sp.coo_matrix((np.ones(a.size, np.float32), (a, b)), shape=(n, n)).tocsr()
    m = ((m + m.T + sp.eye(n)) > 0).astype(np.float32).tocsr()
    shuffle = rng.permutation(n)
    P = sp.coo_matrix((np.ones(n, np.float32), (shuffle, np.arange(n))), shape=(n, n)).tocsr()
    m = (P @ m @ P.T).tocsr()
    m.sort_indices()
    return m


# ---- the row permutation ---------------------------------------------------------------------------------------------------------------
PERMUTE_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 1000)                  # around one and two strides of the wavefront that copies a row
PERMUTE_NS = (1, 2, 3, 4, 5, 8, 1025)


def permute_matrix(n, seed=0):
    """(rowptr int64, col int32, val float32 of any bits) with the row lengths of PERMUTE_LENGTHS: n = 8 holds them all once, n = 1025
    cycles through them in a shuffled order, smaller n take the first of (65, 0, 1000, 1, 64)"""
    rng = np.random.default_rng([n, seed])
    if n <= 5:
        lengths = np.array((65, 0, 1000, 1, 64)[:n], dtype=np.int64)
    elif n == 8:
        lengths = np.array(PERMUTE_LENGTHS, dtype=np.int64)
    else:
        lengths = np.array([PERMUTE_LENGTHS[k % 7] for k in rng.permutation(n)], dtype=np.int64)
        lengths[n // 2] = 1000
    rowptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    nnz = int(rowptr[-1])
    col = rng.integers(0, np.iinfo(np.int32).max, nnz).astype(np.int32)
    val = rng.integers(0, 1 << 32, nnz, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return rowptr, col, val


def permutations(n, seed=1):
    return {"identity": np.arange(n, dtype=np.int32), "reversal": np.arange(n, dtype=np.int32)[::-1].copy(),
            "random": np.random.default_rng([n, seed]).permutation(n).astype(np.int32)}


def permute_rows_reference(rowptr, col, val, perm):
    """numpy fancy indexing: storage row k of the output is row perm[k] of the input, entries untouched"""
    lengths = np.diff(rowptr)[perm]
    out_rowptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    src = np.concatenate([np.arange(rowptr[p], rowptr[p + 1]) for p in perm] + [np.zeros(0, np.int64)]).astype(np.int64)
    return out_rowptr, col[src], val[src]
