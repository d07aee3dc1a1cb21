"""The device LBVH (gsrt_lbvh.hip: build and refit) held to the Karras radix tree at the sizes where its code takes
another path, on degenerate centroid sets and through refits. Every comparison is on integers or exact float32, so
there is no tolerance anywhere. lbvh_ref.check_tree is the checker (items 1 to 6 in its docstring).

The seams and the case that first crosses each:
  kFitLeaves0 = 256 (span and top kernels launched above it)        test_structure[257]
  kSortTile = 4096 (keys per sort block)                            test_structure[4097]
  kFitSpan1 = 16384 (a second level-1 span)                         test_structure[16385]
  nparts capped at 1024 (k_bounds_partial's second trip)            test_structure[262145]
  nblocks > 256 (k_scan_digits: more than one block per thread)     test_structure[1048577]
  kFitSpan2 = 1048576 (a second level-2 span, a top queue)          test_structure[1048577]
2113793 = 2 * 1048576 + 16384 + 257 leaves the last level-2 span, the last level-1 span and the last chunk ragged.
"""
import functools

import numpy as np
import pytest

import gsrt
import lbvh_ref as R

pytestmark = pytest.mark.gpu

SEAMS = [255, 256, 257, 4095, 4096, 4097, 16383, 16384, 16385, 262144, 262145]
LARGE = [1048576, 1048577, 2113793]
KARRAS_MAX = 65537   # lbvh_ref.karras() is a host construction: seconds at a million keys


@pytest.fixture(scope="module")
def rows(ctx):
    """valid GaussParam rows to repeat: the build and the fits read only the AABBs"""
    c, r, s, o, _ = gsrt.synth_cloud(gsrt.SYNTH_COR, 256, 3)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o)
    p, _ = sc.download()
    sc.close()
    return p


# the kinds of cloud() and the axes on which each one's centroids have no extent (None: not stated)
CLOUDS = {"random": (), "identical": (0, 1, 2), "flat1": (1,), "flat2": (0, 2), "repeated": None, "dyadic": (1, 2)}


def _dyadic_half_extents(rng, n):
    return (rng.integers(1, 65, (n, 3)) / 4096).astype(np.float32)     # k 2^-12, k <= 64


@functools.lru_cache(maxsize=None)
def cloud(kind, n):
    """(n, 6) float32 AABBs, finite, half extents positive and different between Gaussians.
    random      centroids uniform in a 6 x 4 x 2 box
    identical   one centroid
    flat1/flat2 zero centroid extent on y / on x and z
    repeated    300 centroids, each about n / 300 times, in shuffled order
    dyadic      x = 2^-k (1.25 + j / 512), k = i % 16, j = i // 16, within (0, 2]: every position once, a sixteenth
                of them in each octave [2^-k, 2^(1 - k)), so every split on an x bit is lopsided; y and z fixed
    Where centroids must coincide exactly, they and the half extents are dyadic numbers narrow enough for c - h, c + h
    and their sum to be exact in float32, so 0.5 (min + max) is c itself."""
    rng = np.random.default_rng([n, sorted(CLOUDS).index(kind)])
    if kind == "random":
        c = (rng.uniform(-1, 1, (n, 3)) * (3, 2, 1)).astype(np.float32)
        h = rng.uniform(1e-3, 2e-2, (n, 3)).astype(np.float32)
    else:
        h = _dyadic_half_extents(rng, n)
        grid = lambda m: (rng.integers(-256, 257, (m, 3)) / 64).astype(np.float32)  # noqa: E731
        if kind == "identical":
            c = np.tile(grid(1), (n, 1))
        elif kind in ("flat1", "flat2"):
            c = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
            for axis in CLOUDS[kind]:
                c[:, axis] = np.float32(0.75)
        elif kind == "repeated":
            c = grid(300)[rng.integers(0, 300, n)]
        elif kind == "dyadic":
            i = np.arange(n)
            x = np.ldexp(1.25 + (i // 16) / 512, -(i % 16))              # exact in float32: 11 bits
            x[0] = 2                                                     # the extent's end: octave k is [2^-k, 2^(1 - k))
            c = np.stack([x, np.full(n, 0.5), np.full(n, 0.5)], axis=1).astype(np.float32)
    a = np.concatenate([c - h, c + h], axis=1).astype(np.float32)
    assert np.isfinite(a).all() and (a[:, 3:] > a[:, :3]).all()
    a.setflags(write=False)
    return a


def centroid_extent(a):
    c = np.float32(0.5) * (a[:, :3] + a[:, 3:])
    return c.max(0) - c.min(0)


def scene_over(ctx, rows, aabbs):
    n = aabbs.shape[0]
    return gsrt.Scene.from_params(ctx, np.resize(rows, (n, 12)), aabbs)


def held(sc, aabbs, codes=None):
    """download the scene's tree and hold it to check_tree over aabbs; returns the download and the checker's result"""
    nodes, gid, msort = sc.bvh_download()
    info = sc.bvh_info()
    assert info["n_internal"] == aabbs.shape[0] - 1
    res = R.check_tree(nodes, gid, msort, aabbs, info["root_box"], info["max_depth"], codes=codes)
    assert info["max_depth"] == res["levels"] <= 64
    return nodes, gid, msort, info, res


def assert_is_karras(msort, res):
    """lo, hi and gamma of the device tree against the independent host construction"""
    lo, hi, gamma = R.karras(R.sort_keys(msort))
    for name, want in (("lo", lo), ("hi", hi), ("gamma", gamma)):
        np.testing.assert_array_equal(res[name], want, err_msg=name)


@pytest.mark.parametrize("n", SEAMS + LARGE)
def test_structure(ctx, rows, n):
    a = cloud("random", n)
    sc = scene_over(ctx, rows, a)
    try:
        sc.build_bvh()
        _, _, msort, _, res = held(sc, a)
        if n <= KARRAS_MAX:
            assert_is_karras(msort, res)
    finally:
        sc.close()


@pytest.mark.parametrize("kind,n", [(k, 4097) for k in ("identical", "flat1", "flat2", "repeated", "dyadic")]
                         + [("repeated", 1048577)])
def test_degenerate_centroids(ctx, rows, kind, n):
    a = cloud(kind, n)
    # the case is what it says: the extents that must vanish do, the codes repeat as they should
    ext = centroid_extent(a)
    codes = R.morton(a)
    if CLOUDS[kind] is not None:
        flat = np.isin(np.arange(3), CLOUDS[kind])
        assert (ext[flat] == 0).all() and (ext[~flat] > 0).all()
    if kind == "identical":
        assert (codes == 0).all()
    if kind == "repeated":
        s = np.sort(codes)
        assert np.unique(codes).size <= 300
        assert (s[4095:-1:4096] == s[4096::4096]).any()       # a run of equal codes lies across a sort-block boundary
    if kind == "dyadic":
        x = np.float32(0.5) * (a[:, 0] + a[:, 3])
        assert np.unique(x).size == n                          # one Gaussian per position
        top = np.arange(n) % 16 == 0                           # the octave [1, 2): the upper half of the extent ...
        mid = 0.5 * (float(x.min()) + float(x.max()))
        assert x[top].min() > 1.1 * mid and x[~top].max() < 0.9 * mid
        np.testing.assert_array_equal(codes >> 29 == 1, top)   # ... so the highest x bit is theirs alone
    sc = scene_over(ctx, rows, a)
    try:
        sc.build_bvh()
        _, _, msort, _, res = held(sc, a)
        if n <= KARRAS_MAX:
            assert_is_karras(msort, res)
        if kind == "dyadic":  # the root sets one sixteenth aside, and so on down the octaves: deeper than a balanced tree
            assert res["gamma"][0] + 1 == n - top.sum()
            assert res["levels"] > int(np.ceil(np.log2(n))) + 1
    finally:
        sc.close()


def shifted(a, seed):
    d = np.random.default_rng(seed).normal(0, 1e-2, (a.shape[0], 3)).astype(np.float32)
    a2 = a.copy()
    a2[:, :3] += d
    a2[:, 3:] += d
    return a2


@pytest.mark.parametrize("n", [16385, 1048577])
def test_refit(ctx, rows, n):
    """Two refits in a row, each held to items 1 to 5 over the moved AABBs (the order is the build's: a refit keeps
    the topology), then a refit back: every node word outside the key slots is the fresh build's again. A count or a
    queue left non-zero by one fit would fit a node early, or twice, in the next."""
    a = cloud("random", n)
    codes = R.morton(a)
    sc = scene_over(ctx, rows, a)
    try:
        sc.build_bvh()
        nodes0, gid0, msort0 = sc.bvh_download()
        info0 = sc.bvh_info()
        for seed in (11, 12):
            a2 = shifted(a, seed)
            sc.refit_bvh(a2)
            nodes, gid, msort, _, _ = held(sc, a2, codes=codes)
            np.testing.assert_array_equal(gid, gid0)
            np.testing.assert_array_equal(msort, msort0)
            np.testing.assert_array_equal(nodes[:, [R.L_REF, R.R_REF]], nodes0[:, [R.L_REF, R.R_REF]])
        sc.refit_bvh(a)
        nodes, gid, msort = sc.bvh_download()
        info = sc.bvh_info()
        np.testing.assert_array_equal(nodes[:, R.TREE_WORDS], nodes0[:, R.TREE_WORDS])
        np.testing.assert_array_equal(info["root_box"].view(np.uint32), info0["root_box"].view(np.uint32))
        np.testing.assert_array_equal(gid, gid0)
        np.testing.assert_array_equal(msort, msort0)
        if n <= KARRAS_MAX:  # the large tree itself is test_structure's (the same cloud)
            R.check_tree(nodes, gid, msort, a, info["root_box"], info["max_depth"])
    finally:
        sc.close()


def test_refit_shrinks_every_ancestor(ctx, rows):
    """One AABB grows a hundredfold and shrinks back: a fit that only ever enlarged boxes would render the same frames.
    Grown, every ancestor's box holds it exactly; shrunk back, every word is the fresh build's."""
    n = 16385
    a = cloud("random", n)
    codes = R.morton(a)
    sc = scene_over(ctx, rows, a)
    try:
        sc.build_bvh()
        nodes0, gid0, msort0, info0, res0 = held(sc, a)
        g = int(gid0[n // 2 + 100])                      # a leaf in the middle of a chunk of a middle span
        big = a.copy()
        big[g, :3] -= 50
        big[g, 3:] += 50
        sc.refit_bvh(big)
        nodes, gid, msort, info, res = held(sc, big, codes=codes)
        np.testing.assert_array_equal(info["root_box"], big[g])       # it dwarfs the cloud
        at = n // 2 + 100
        above = (res0["lo"] <= at) & (res0["hi"] >= at)                # the leaf's ancestors: their runs hold it
        left = res0["gamma"] >= at                                     # ... in the left child's run, else the right's
        lo, hi = res0["lo"][above], res0["hi"][above]
        # fitted by every launch: ancestors inside a chunk of 256 leaves, across chunks inside a span of 16384, and above
        in_chunk, in_span = lo // 256 == hi // 256, lo // 16384 == hi // 16384
        assert above[0] and in_chunk.any() and (in_span & ~in_chunk).any() and (~in_span).any()

        def slots(nd):
            fl = nd.view(np.float32)
            return np.where(left[:, None], fl[:, R.L_BOX], fl[:, R.R_BOX])[above]

        assert (slots(nodes) == big[g]).all()
        sc.refit_bvh(a)
        nodes, gid, msort, info, _ = held(sc, a)
        np.testing.assert_array_equal(nodes[:, R.TREE_WORDS], nodes0[:, R.TREE_WORDS])
        np.testing.assert_array_equal(info["root_box"].view(np.uint32), info0["root_box"].view(np.uint32))
        assert (np.abs(slots(nodes)) < 4).all()                        # the cloud lies within +-3.02: no trace of the 50
    finally:
        sc.close()
