"""The LBVH checker must be able to fail (CPU). Trees are built on the host from lbvh_ref.karras() and exact unions;
check_tree accepts them and rejects each single mutation, naming the node. karras() itself is compared with the plain
recursive construction, so the reference is checked twice.

Which of check_tree's items catches which mutation:
  box_inward, box_outward   5 (the stored child box is not the exact union)
  children_swapped          3 (hi(left) + 1 != lo(right))
  split_moved               4 (the split's keys share more bits than the run's ends)
  children_exchanged        3 (a node's index is not an end of its run)
  gid_unstable              1 (gid is not the stable argsort)
  leaf_duplicated           2 (a leaf referenced twice, another never)
  node_duplicated           2 (an internal node referenced twice)
  root_box_wrong            5 (the root box is not the union of the root's children)
  depth_over, depth_under   6
"""
import functools

import numpy as np
import pytest

import lbvh_ref as R

SIZES = [2, 3, 17, 257, 1000, 4097]
KINDS = ["random", "equal", "runs"]


def make_aabbs(kind, n, seed=0):
    """random: distinct centroids. equal: one centroid. runs: about n / 8 centroids, each repeated, in shuffled order.
    The repeated centroids and their half extents are small dyadic numbers, so 0.5 (min + max) is the centroid exactly
    and equal centroids get equal codes. Half extents always differ between Gaussians."""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    if kind == "random":
        c = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
        h = rng.uniform(0.01, 0.05, (n, 3)).astype(np.float32)
    else:
        m = 1 if kind == "equal" else n // 8 + 1
        grid = (rng.integers(-256, 257, (m, 3)) / 64).astype(np.float32)
        c = grid[rng.integers(0, m, n)]
        h = (rng.integers(1, 65, (n, 3)) / 4096).astype(np.float32)
    return np.concatenate([c - h, c + h], axis=1).astype(np.float32)


def nodes_from(lo, hi, gamma, gid):
    """the node words (boxes zero) of a tree given by every node's run and split"""
    ni = lo.shape[0]
    nodes = np.zeros((ni, 16), np.uint32)
    nodes[:, R.L_REF] = np.where(lo == gamma, R.LEAF | gid[gamma], gamma)
    nodes[:, R.R_REF] = np.where(hi == gamma + 1, R.LEAF | gid[gamma + 1], gamma + 1)
    return nodes


def fit(nodes, aabbs):
    """exact bottom-up boxes, one node at a time (shares nothing with check_tree's level passes); returns the root box
    and the depth as Scene.bvh_info counts it (root 1, a leaf one more than its parent)"""
    fl = nodes.view(np.float32)
    depth = {0: 1}
    post, stack = [], [0]
    while stack:
        i = stack.pop()
        post.append(i)
        for w in (R.L_REF, R.R_REF):
            if not nodes[i, w] & R.LEAF:
                depth[int(nodes[i, w])] = depth[i] + 1
                stack.append(int(nodes[i, w]))
    assert len(post) == nodes.shape[0]
    box = {}
    for i in reversed(post):
        b = []
        for w, cols in ((R.L_REF, R.L_BOX), (R.R_REF, R.R_BOX)):
            r = int(nodes[i, w])
            b.append(aabbs[r & 0x7FFFFFFF] if r & R.LEAF else box[r])
            fl[i, cols] = b[-1]
        box[i] = np.concatenate([np.minimum(b[0][:3], b[1][:3]), np.maximum(b[0][3:], b[1][3:])])
    return box[0].astype(np.float32), max(depth.values()) + 1


def tree_over(aabbs):
    codes = R.morton(aabbs)
    gid = np.argsort(codes, kind="stable").astype(np.uint32)
    msort = codes[gid]
    lo, hi, gamma = R.karras(R.sort_keys(msort))
    nodes = nodes_from(lo, hi, gamma, gid)
    root, depth = fit(nodes, aabbs)
    return dict(nodes=nodes, gid=gid, morton_sorted=msort, aabbs=aabbs, root_box=root, max_depth=depth,
                lo=lo, hi=hi, gamma=gamma)


@functools.lru_cache(maxsize=None)
def _tree(kind, n):
    return tree_over(make_aabbs(kind, n))


def tree(kind, n):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _tree(kind, n).items()}


def check(t):
    return R.check_tree(t["nodes"], t["gid"], t["morton_sorted"], t["aabbs"], t["root_box"], t["max_depth"])


def _ulp(x, up):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf))


# ---- the mutations: each returns (mutated tree, the id the message must name) or None where it does not apply


def _box_move(t, rng, outward):
    fl = t["nodes"].view(np.float32)
    node = int(rng.integers(0, fl.shape[0]))
    w = int(rng.choice(R.L_BOX + R.R_BOX))
    is_lo = w % 8 < 3
    fl[node, w] = _ulp(fl[node, w], up=(is_lo != outward))
    return t, node


def box_inward(t, rng):
    return _box_move(t, rng, False)


def box_outward(t, rng):
    return _box_move(t, rng, True)


def children_swapped(t, rng):
    node = int(rng.integers(0, t["nodes"].shape[0]))
    row = t["nodes"][node].copy()
    t["nodes"][node, R.L_BOX + [R.L_REF]] = row[R.R_BOX + [R.R_REF]]
    t["nodes"][node, R.R_BOX + [R.R_REF]] = row[R.L_BOX + [R.L_REF]]
    return t, node


def split_moved(t, rng):
    wide = np.flatnonzero(t["hi"] - t["lo"] >= 2)
    if not wide.size:
        return None
    node = int(rng.choice(wide))
    a, b, g = int(t["lo"][node]), int(t["hi"][node]), int(t["gamma"][node])
    g2 = g + 1 if g + 1 < b else g - 1
    lo, hi, gamma = R.karras_recursive(R.sort_keys(t["morton_sorted"]), {(a, b): g2})
    t["nodes"] = nodes_from(lo, hi, gamma, t["gid"])
    t["root_box"], t["max_depth"] = fit(t["nodes"], t["aabbs"])
    return t, node


def children_exchanged(t, rng):
    """internal nodes x and y change places (rows and the references to them): the same tree, leaf order and splits, but
    node y now covers x's run, of which y is no end"""
    lo, hi = t["lo"], t["hi"]
    ni = lo.shape[0]
    for _ in range(1000):
        if ni < 3:
            return None
        x, y = (int(v) for v in rng.choice(np.arange(1, ni), 2, replace=False))
        if y in (lo[x], hi[x]) or x in (lo[y], hi[y]):
            continue
        nodes = t["nodes"]
        refs = nodes[:, [R.L_REF, R.R_REF]]
        to_x, to_y = refs == x, refs == y
        refs[to_x], refs[to_y] = y, x
        nodes[:, [R.L_REF, R.R_REF]] = refs
        nodes[[x, y]] = nodes[[y, x]]
        # the deeper of the two subtrees is met first, on the way up from the deepest level
        dx, dy = (int(((lo <= lo[v]) & (hi >= hi[v])).sum()) for v in (x, y))  # ancestors, itself included
        return t, (y if dx > dy else x if dy > dx else min(x, y))
    return None


def gid_unstable(t, rng):
    m = t["morton_sorted"]
    ties = np.flatnonzero(m[1:] == m[:-1])
    if not ties.size:
        return None
    k = int(rng.choice(ties))
    t["gid"][[k, k + 1]] = t["gid"][[k + 1, k]]
    # the tree over the swapped order, refitted: only the order itself is wrong
    t["nodes"] = nodes_from(t["lo"], t["hi"], t["gamma"], t["gid"])
    t["root_box"], t["max_depth"] = fit(t["nodes"], t["aabbs"])
    return t, k


def leaf_duplicated(t, rng):
    refs = t["nodes"][:, [R.L_REF, R.R_REF]]
    at = np.argwhere(refs & R.LEAF)
    node, side = at[rng.integers(0, at.shape[0])]
    old = int(refs[node, side] & 0x7FFFFFFF)
    new = (old + 1 + int(rng.integers(0, t["gid"].shape[0] - 1))) % t["gid"].shape[0]
    t["nodes"][node, (R.L_REF, R.R_REF)[side]] = R.LEAF | new
    return t, min(old, new)


def node_duplicated(t, rng):
    refs = t["nodes"][:, [R.L_REF, R.R_REF]]
    at = np.argwhere(refs & R.LEAF)
    ni = refs.shape[0]
    if ni < 2:
        return None
    node, side = at[rng.integers(0, at.shape[0])]
    twice = int(rng.integers(1, ni))
    t["nodes"][node, (R.L_REF, R.R_REF)[side]] = twice
    return t, twice


def root_box_wrong(t, rng):
    k = int(rng.integers(0, 6))
    t["root_box"][k] = _ulp(t["root_box"][k], up=bool(rng.integers(0, 2)))
    return t, None


def depth_over(t, rng):
    t["max_depth"] += 1
    return t, None


def depth_under(t, rng):
    t["max_depth"] -= 1
    return t, None


MUTATIONS = [box_inward, box_outward, children_swapped, split_moved, children_exchanged, gid_unstable, leaf_duplicated,
             node_duplicated, root_box_wrong, depth_over, depth_under]
MESSAGE = {
    "box_inward": "box is not the exact union", "box_outward": "box is not the exact union",
    "children_swapped": "do not adjoin", "split_moved": "split is not Karras's",
    "children_exchanged": "not an end of its leaf run", "gid_unstable": "not the stable argsort",
    "leaf_duplicated": "leaf not referenced exactly once", "node_duplicated": "internal node not referenced exactly once",
    "root_box_wrong": "root box", "depth_over": "max_depth", "depth_under": "max_depth",
}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_check_tree_accepts_the_reference_tree(kind, n):
    t = tree(kind, n)
    got = check(t)
    for k in ("lo", "hi", "gamma"):
        np.testing.assert_array_equal(got[k], t[k])
    assert got["levels"] == t["max_depth"] <= 64
    if kind == "equal":
        assert (t["morton_sorted"] == 0).all()
    if kind == "runs" and n >= 17:
        assert np.unique(t["morton_sorted"]).size < n


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mutation", MUTATIONS, ids=lambda f: f.__name__)
def test_check_tree_rejects(mutation, kind, n):
    applied = 0
    for trial in range(3):  # three places in the tree
        rng = np.random.default_rng([trial, n, KINDS.index(kind), MUTATIONS.index(mutation)])
        m = mutation(tree(kind, n), rng)
        if m is None:
            continue
        applied += 1
        t, where = m
        with pytest.raises(R.TreeError, match=MESSAGE[mutation.__name__]) as e:
            check(t)
        assert "first at" in str(e.value) or "node 0" in str(e.value) or "max_depth" in str(e.value), str(e.value)
        if where is not None:
            assert f"first at {where} " in str(e.value), (where, str(e.value))
    # where a mutation cannot be made: too few nodes, or no two equal codes
    impossible = {"split_moved": n < 3, "children_exchanged": n < 4, "node_duplicated": n < 3,
                  "gid_unstable": kind == "random"}
    assert applied == (0 if impossible.get(mutation.__name__, False) else 3)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_karras_equals_the_recursive_construction(kind, n):
    t = tree(kind, n)
    keys = R.sort_keys(t["morton_sorted"])
    for got, want in zip(R.karras(keys), R.karras_recursive(keys)):
        np.testing.assert_array_equal(got, want)


def test_karras_on_full_width_keys():
    """keys that differ in any of the 64 bits, and runs that differ only in the lowest"""
    rng = np.random.default_rng(5)
    for n in (2, 3, 64, 999):
        k = rng.integers(0, 2 ** 63, n, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, n, dtype=np.uint64)
        k >>= rng.integers(0, 64, n, dtype=np.uint64)
        k = np.unique(np.concatenate([k, k ^ np.uint64(1), np.uint64([0, 2 ** 64 - 1])]))
        for got, want in zip(R.karras(k), R.karras_recursive(k)):
            np.testing.assert_array_equal(got, want)


def test_clz64():
    rng = np.random.default_rng(9)
    v = rng.integers(0, 2 ** 63, 4096, dtype=np.uint64) >> rng.integers(0, 64, 4096, dtype=np.uint64)
    v = np.concatenate([v, np.uint64([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 53 + 1, 2 ** 63, 2 ** 64 - 1])])
    np.testing.assert_array_equal(R.clz64(v), [64 - int(x).bit_length() for x in v])


def test_one_leaf():
    a = make_aabbs("random", 1)
    z = np.zeros(1, np.uint32)
    assert R.check_tree(np.zeros((0, 16), np.uint32), z, z, a, a[0], 1)["levels"] == 1
    with pytest.raises(R.TreeError, match="root box"):
        R.check_tree(np.zeros((0, 16), np.uint32), z, z, a, a[0] + np.float32(1), 1)
    with pytest.raises(R.TreeError, match="max_depth"):
        R.check_tree(np.zeros((0, 16), np.uint32), z, z, a, a[0], 2)


def test_signed_zero_is_one_value():
    """a bound at zero: the stored box may carry either zero, and nothing else but the union's own bits"""
    a = make_aabbs("random", 17)
    a[:, 0] = np.minimum(a[:, 0], 0)
    a[3, 0] = 0.0
    a[5, 0] = -0.0
    t = tree_over(a)
    check(t)
    fl = t["nodes"].view(np.float32)
    zero = fl == 0
    assert zero[:, R.L_BOX + R.R_BOX].any()
    t["nodes"][zero & (np.arange(16) % 4 != 3)] ^= np.uint32(R.LEAF)      # every zero box float changes sign
    check(t)
    node, w = np.argwhere(zero & (np.arange(16) % 4 != 3))[0]
    t["nodes"][node, w] = 1                                              # the smallest denormal
    with pytest.raises(R.TreeError, match=f"box is not the exact union.*first at {node} "):
        check(t)
