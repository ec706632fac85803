"""rc_bucket_plan against oracle/plan_oracle.py at the batch and bucket sizes where the loading of csrc/bucket_plan.hip can go wrong.

plan_count_kernel and plan_scatter_kernel request a thread's 16 raw ids together and turn them into keys afterwards; the scatter
requests the bucket totals and its tile's histogram column in the same trip, in front of its first barrier.  What can go wrong
there: the guard of a load (positions past the end of the batch, the ragged last tile, the seam between list a and list b inside
a tile), padding (negative) ids, the surplus workgroups of the grid (8 * ceil(tiles / 8)), the column of the last tile, and either
geometry's instantiation (id-range buckets / hashed buckets).  plan_bucket_kernel reads what the scatter wrote, in batches of 2,048
keys (count pass) and 1,024 keys (ordered pass): the sized buckets sit at the ends of those batches (6,144 keys = three and six
whole batches), at single rounds of 64 lanes, and past 32,768 keys (32-bit LDS cells).  Integer work: every comparison is exact.

The buckets are built by hand: the id range is chosen so that plan_geometry takes id-range buckets of a known width, and every
sized bucket gets exactly the stated number of keys, spread over the whole batch, a few ids each, so that rows with several
occurrences straddle rounds, batches and tiles.  _geometry() restates plan_geometry's rule so that the construction can assert the
width it aims at; it is a statement about the inputs, the comparison with the oracle does not depend on it."""
import numpy as np
import pytest
import torch

from oracle import plan_oracle as PO

pytestmark = pytest.mark.gpu

PRE = 6144                 # three whole batches of the bucket kernel's count pass (2,048 keys), six of its ordered pass (1,024)
TILE = 8192                # positions per workgroup of the count / scatter kernels (plan.hpp: kPlanTile)


@pytest.fixture(scope="module")
def eng(cuda):
    from rechorus_amd import engine
    return engine


def _geometry(n, ra, rb):
    """plan_geometry (bucket_plan.hip) restated for the automatic mode: -> ("hashed" | "narrow" | "wide", shift)"""
    nbk = lambda sh: -(-ra // (1 << sh)) + (-(-rb // (1 << sh)) if rb else 0)
    if nbk(13) > 4096 or ra + rb > 16 * n:
        return "hashed", 0
    if n >= 4 * (ra + rb):
        sh = 0
        while nbk(sh) > 4096:
            sh += 1
        if sh <= 5:
            return "narrow", sh
    want = min(max(n // 8192, 128), 1024)
    sh = 13
    while sh > 8 and nbk(sh) < want and nbk(sh - 1) <= 4096:
        sh -= 1
    while nbk(sh) > 4096:
        sh += 1
    return "wide", sh


def _bucket_ids(rng, bucket, shift, count, kind):
    """`count` ids of id-range bucket `bucket` (table-local ids bucket << shift ...)"""
    width = 1 << shift
    base = bucket << shift
    if kind == "one_row":          # one row alone: every round of 64 lanes holds the same row
        return np.full(count, base + 5, dtype=np.int64)
    if kind == "row_run":          # one row fills whole rounds in the middle of the bucket's keys, other rows before and after
        head = base + rng.integers(0, width, size=37)
        tail = base + rng.integers(0, width, size=count - 37 - 300)
        return np.concatenate([head, np.full(300, base + 9), tail]).astype(np.int64)
    # a few keys per id (rows of 1 .. ~12 occurrences), first and last id of the bucket among them
    ids = base + rng.integers(0, max(min(width, count // 3), 1), size=count)
    if count >= 2:
        ids[0], ids[-1] = base, base + width - 1
    return ids.astype(np.int64)


def _batch(rng, shift, sized_a, sized_b, n_total, nb_a, nb_b, pad_bucket):
    """-> (ids_a, ids_b, range_a, range_b).  sized_x: [(bucket, count, kind)]; the remaining positions of list a draw from the
    buckets no sized bucket uses.  The keys of a bucket keep their order (its rows' occurrences ascend with the position),
    buckets are interleaved at random over the batch; `pad_bucket` (list a) gets a negative id in front of and behind its keys
    number 256 k - 1 and 256 k -- padding positions take no part, so the bucket's keys stay what they were."""
    def side(sized, nb, n_side):
        parts = [_bucket_ids(rng, b, shift, c, k) for b, c, k in sized]
        used = {b for b, _, _ in sized}
        free = np.array([b for b in range(nb) if b not in used], dtype=np.int64)
        n_fill = n_side - sum(len(p) for p in parts)
        assert n_fill >= 0
        if n_fill:
            parts.append((rng.choice(free, size=n_fill) << shift) + rng.integers(0, 1 << shift, size=n_fill))
        # random interleaving that keeps every part's own order: a stable sort of the part labels by random slot
        label = np.concatenate([np.full(len(p), i) for i, p in enumerate(parts)])
        label = label[rng.permutation(len(label))]
        out = np.empty(len(label), dtype=np.int64)
        for i, p in enumerate(parts):
            out[label == i] = p
        return out
    n_b = sum(c for _, c, _ in sized_b) + 50
    a = side(sized_a, nb_a, n_total - n_b)
    b = side(sized_b, nb_b, n_b)
    if pad_bucket is not None:
        at = np.flatnonzero((a >> shift) == pad_bucket)
        q = -(-len(at) // 256) * 64
        edge = [i for w in (1, 2, 3) for i in (w * q - 1, w * q) if 0 <= i < len(at)]
        where = np.concatenate([at[edge], at[edge] + 1])
        a = np.insert(a, where, -1)
    return a, b, nb_a << shift, nb_b << shift


def _check(eng, cuda, ids_a, range_a, ids_b, range_b, list_single_a):
    a = torch.from_numpy(np.ascontiguousarray(ids_a, dtype=np.int64)).to(cuda)
    b = None if ids_b is None else torch.from_numpy(np.ascontiguousarray(ids_b, dtype=np.int64)).to(cuda)
    out = eng.bucket_plan(a, range_a, b, range_b, list_single_a=list_single_a)
    want_a, want_b, want_single = PO.bucket_plan(ids_a, ids_b, list_single_a)
    occ = out["occ"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    for rows, want, name in ((out["rows_a"], want_a, "a"), (out["rows_b"], want_b, "b")):
        r = rows.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        assert len(r) == len(want), f"list {name}: {len(r)} rows listed, {len(want)} expected"
        assert len(np.unique(r[:, 0])) == len(r), f"list {name}: a row is listed twice"
        assert np.all(r[:, 3] == 0)
        for row, start, n, _ in r:
            got, exp = occ[start:start + n], want[int(row)]
            assert np.array_equal(got, exp), f"list {name} row {row}: positions {got[:8]}.. != {exp[:8]}.."
    if list_single_a:
        assert out["single"] is None
    else:
        assert np.array_equal(out["single"].cpu().numpy(), want_single)


# key counts of the sized buckets: empty, one key, around one round of 64, a count that is no multiple of 4 or of 256,
# one below / at / one above whole batches of both loops of the bucket kernel, then one and two batches of the ordered loop more
# plus one key (the second: one batch of the count loop more plus one key)
SIZES = [0, 1, 63, 64, 65, 1001, PRE - 1, PRE, PRE + 1, PRE + 1024 + 1, PRE + 2048 + 1]


@pytest.mark.parametrize("list_single_a", [True, False])
@pytest.mark.parametrize("shift", [10, 8])   # 1,024-id buckets: 16-bit LDS cells; 256-id buckets: the 32-bit (WIDE) instantiation
def test_sized_buckets_nine_tiles(shift, list_single_a, cuda, eng):
    """every bucket size of SIZES on the item side, one row alone in its bucket (ten whole rounds of one row), a row that fills
    whole rounds between other rows, three sized buckets on the user side (list b), negative ids beside keys of the 1,001-key bucket
    and at the wave and tile seams of the batch (positions 1,023 / 1,024 and 8,191 / 8,192); 9 tiles: the scatter grid is 16
    workgroups, 7 of them surplus, the last tile (8) is a ragged one, the seam between the two lists lies inside tile 7"""
    rng = np.random.default_rng(100 + shift)
    nb_a, nb_b = 128, 4
    sized_a = [(2 + i, c, "mixed") for i, c in enumerate(SIZES)] + [(20, 640, "one_row"), (21, 900, "row_run")]
    sized_b = [(0, 65, "mixed"), (1, 1001, "mixed"), (3, PRE + 1, "mixed")]        # (bucket 2 of list b: the 50 other users)
    n_total = 8 * TILE + 4000
    a, b, ra, rb = _batch(rng, shift, sized_a, sized_b, n_total, nb_a, nb_b, pad_bucket=2 + SIZES.index(1001))
    a = np.insert(a, [1023, 1024, 8191, 8192], -1)
    assert -(-(len(a) + len(b)) // TILE) == 9 and len(a) % TILE != 0
    assert _geometry(len(a) + len(b), ra, rb) == ("wide", shift)
    for bkt, c, _ in sized_a:
        assert int(((a >= 0) & ((a >> shift) == bkt)).sum()) == c
    for bkt, c, _ in sized_b:
        assert int(((b >> shift) == bkt).sum()) == c
    assert int((a < 0).sum()) == 16
    _check(eng, cuda, a, ra, b, rb, list_single_a)


@pytest.mark.parametrize("list_single_a", [True, False])
def test_sized_buckets_one_tile(list_single_a, cuda, eng):
    """the same kinds of bucket in a batch of ONE tile (scatter grid: 8 workgroups, 7 surplus; tile 0 is the last tile)"""
    rng = np.random.default_rng(7)
    shift, nb_a, nb_b = 9, 126, 2
    sized_a = [(1, 0, "mixed"), (2, 1, "mixed"), (3, 63, "mixed"), (4, 64, "mixed"), (5, 65, "mixed"), (6, 1001, "mixed"),
               (7, PRE + 1, "mixed")]
    sized_b = [(1, 65, "mixed")]
    a, b, ra, rb = _batch(rng, shift, sized_a, sized_b, 8100, nb_a, nb_b, pad_bucket=6)
    assert len(a) + len(b) <= TILE
    assert _geometry(len(a) + len(b), ra, rb) == ("wide", shift)
    for bkt, c, _ in sized_a:
        assert int(((a >= 0) & ((a >> shift) == bkt)).sum()) == c
    _check(eng, cuda, a, ra, b, rb, list_single_a)


@pytest.mark.parametrize("list_single_a", [True, False])
@pytest.mark.parametrize("table", ["200k_rows", "64_rows"])
def test_bucket_past_32768_keys(table, list_single_a, cuda, eng):
    """40,000 positions on 64 rows.  In a table of 200,000 rows they are ONE id-range bucket of >= 32,768 keys, which the 32-bit
    (WIDE) instantiation takes.  (A table of 64 rows alone is a dense batch:
    plan_geometry gives it one-id buckets and the narrow kernel -- kept as a case, it is what the size describes.)"""
    rng = np.random.default_rng(40_000)
    hot = rng.integers(0, 64, size=40_000).astype(np.int64)
    if table == "64_rows":
        a, ra, b, rb = hot, 64, rng.integers(0, 5, size=30).astype(np.int64), 5
        assert _geometry(len(a) + len(b), ra, rb)[0] == "narrow"
    else:
        ra, rb = 200_000, 3_000
        a = np.concatenate([hot, rng.integers(0, ra, size=20_000)])
        rng.shuffle(a)
        b = rng.integers(0, rb, size=500).astype(np.int64)
        kind, shift = _geometry(len(a) + len(b), ra, rb)
        assert kind == "wide" and shift > 8 and int((a >> shift == 0).sum()) >= 32_768
    _check(eng, cuda, a, ra, b, rb, list_single_a)


@pytest.mark.parametrize("list_single_a", [True, False])
@pytest.mark.parametrize("tiles", [1, 9])
def test_hashed_geometry_one_and_nine_tiles(tiles, list_single_a, cuda, eng):
    """the hashed instantiations of the count and scatter kernels (id space wider than 16 ids per key): one tile and nine, a
    ragged last tile that holds the seam between the lists, negative ids at the wave and tile seams, ids that repeat"""
    rng = np.random.default_rng(900 + tiles)
    n = 7000 if tiles == 1 else 8 * TILE + 3000
    ra, rb = 50_000_000, 3_000_000
    n_b = 300
    a = rng.integers(0, ra, size=n - n_b)
    a[rng.integers(0, len(a), size=len(a) // 5)] = a[:len(a) // 5]        # rows with several occurrences
    a[[0, 63, 64, 1023, 1024, len(a) - 1]] = -1
    if tiles == 9:
        a[[8191, 8192, 8 * TILE - 1, 8 * TILE]] = -1
    b = rng.integers(0, rb, size=n_b)
    b[[0, n_b - 1]] = -1
    assert -(-(len(a) + len(b)) // TILE) == tiles and _geometry(len(a) + len(b), ra, rb)[0] == "hashed"
    _check(eng, cuda, a, ra, b, rb, list_single_a)
