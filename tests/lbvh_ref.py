"""The LBVH's reference and checker (numpy only; shared by test_lbvh_ref.py, test_lbvh_seams_gpu.py and
test_bvh_gpu.py).

morton(aabbs)     the 30-bit Morton codes of the AABB centroids, float32 operation by operation as k_morton has them
karras(keys)      the radix tree over sorted, distinct 64-bit keys by Karras's searches (2012), vectorised over the nodes
check_tree(...)   everything a downloaded tree is held to; one numpy step per tree level, no per-node Python loop

A node is 16 uint32 words: [l_lo 3, l_ref, l_hi 3, r_ref, r_lo 3, l_key, r_hi 3, r_key]. A reference with kLeafBit set is
a leaf (the Gaussian's id in the low bits), any other an internal node's index. The sort key of sorted position k is
code[k] << 32 | k, so keys are distinct and the radix tree over them is unique.
"""
import numpy as np

LEAF = 0x80000000
L_REF, R_REF = 3, 7
L_BOX = [0, 1, 2, 4, 5, 6]
R_BOX = [8, 9, 10, 12, 13, 14]
KEY_WORDS = [11, 15]                      # l_key / r_key: the projection's, never examined here
TREE_WORDS = [w for w in range(16) if w not in KEY_WORDS]


def _expand(v):
    v = v.astype(np.uint64)
    v = (v * 0x00010001) & 0xFF0000FF
    v = (v * 0x00000101) & 0x0F00F00F
    v = (v * 0x00000011) & 0xC30C30C3
    v = (v * 0x00000005) & 0x49249249
    return v.astype(np.uint32)


def _morton_np(aabbs):
    a = aabbs.astype(np.float32)
    c = np.float32(0.5) * (a[:, :3] + a[:, 3:])
    lo, hi = c.min(0), c.max(0)
    ext = hi - lo
    u = np.where(ext > 0, (c - lo) / np.where(ext > 0, ext, 1), np.float32(0)).astype(np.float32)
    q = np.clip(u * np.float32(1024.0), 0, 1023).astype(np.uint32)
    return (_expand(q[:, 0]) << 2) | (_expand(q[:, 1]) << 1) | _expand(q[:, 2])


def morton(aabbs):
    return _morton_np(aabbs)


def sort_keys(codes_sorted):
    """code[k] << 32 | k over the sorted codes"""
    c = np.asarray(codes_sorted, np.uint64)
    return (c << np.uint64(32)) | np.arange(c.shape[0], dtype=np.uint64)


def _bitlen32(v):
    # exact: every uint32 is a float64, and frexp's exponent of a positive integer is its bit length
    return np.frexp(v.astype(np.float64))[1].astype(np.int64)


def clz64(x):
    """leading zeros of uint64 values (64 at zero)"""
    x = np.asarray(x, np.uint64)
    hi = (x >> np.uint64(32)).astype(np.uint32)
    lo = (x & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return 64 - np.where(hi != 0, 32 + _bitlen32(hi), _bitlen32(lo))


def karras(keys):
    """The radix tree over sorted, distinct uint64 keys: (lo, hi, gamma), each (n - 1,) int64. Internal node i covers
    the sorted positions [lo[i], hi[i]], with i == lo[i] or i == hi[i]; its left child covers [lo[i], gamma[i]] and its
    right child [gamma[i] + 1, hi[i]]. A child that covers one position is that leaf; otherwise it is the internal node
    gamma[i] (left) or gamma[i] + 1 (right). Node 0 is the root."""
    keys = np.asarray(keys, np.uint64)
    n = keys.shape[0]
    if n < 2:
        z = np.zeros(0, np.int64)
        return z, z.copy(), z.copy()
    assert (keys[1:] > keys[:-1]).all(), "karras(): the keys must be sorted and distinct"
    i = np.arange(n - 1, dtype=np.int64)

    def delta(a, b):  # common prefix length of keys a and b; -1 where b is out of range
        ok = (b >= 0) & (b < n)
        return np.where(ok, clz64(keys[a] ^ keys[np.where(ok, b, 0)]), -1)

    d = np.where(delta(i, i + 1) > delta(i, i - 1), 1, -1).astype(np.int64)
    dmin = delta(i, i - d)
    lmax = np.full(n - 1, 2, np.int64)
    while True:  # the range's other end lies within lmax: doubling, log n steps
        grow = delta(i, i + lmax * d) > dmin
        if not grow.any():
            break
        lmax = np.where(grow, lmax * 2, lmax)
    length = np.zeros(n - 1, np.int64)
    t = int(lmax.max()) >> 1
    while t >= 1:  # binary search for the other end
        take = (t < lmax) & (delta(i, i + (length + t) * d) > dmin)
        length = np.where(take, length + t, length)
        t >>= 1
    j = i + length * d
    dnode = delta(i, j)
    s = np.zeros(n - 1, np.int64)
    step = length.copy()
    live = np.ones(n - 1, bool)
    while live.any():  # binary search for the split: the last position that shares more than dnode bits with i
        step = np.where(live, (step + 1) >> 1, step)
        ns = s + step
        take = live & (ns < length) & (delta(i, i + ns * d) > dnode)
        s = np.where(take, ns, s)
        live &= step > 1
    gamma = i + s * d + np.minimum(d, 0)
    return np.minimum(i, j), np.maximum(i, j), gamma


def karras_recursive(keys, override=None):
    """The same tree by the plain definition: a range splits where its highest differing key bit goes from 0 to 1.
    For small n (a Python loop per node). The runs in `override` ({(lo, hi): gamma}) split where it says instead:
    children take Karras's indices (gamma, gamma + 1) all the same, so the result is a valid binary tree either way."""
    override = override or {}
    keys = [int(k) for k in keys]
    n = len(keys)
    lo, hi, gamma = (np.full(max(n - 1, 0), -1, np.int64) for _ in range(3))
    if n < 2:
        return lo, hi, gamma
    stack = [(0, 0, n - 1)]
    while stack:
        node, a, b = stack.pop()
        if (a, b) in override:
            g = override[(a, b)]
        else:
            bit = (keys[a] ^ keys[b]).bit_length() - 1
            g = a
            while (keys[g + 1] >> bit) & 1 == 0:
                g += 1
        assert lo[node] < 0, "a node index was given twice"
        lo[node], hi[node], gamma[node] = a, b, g
        if g > a:
            stack.append((g, a, g))
        if g + 1 < b:
            stack.append((g + 1, g + 1, b))
    return lo, hi, gamma


class TreeError(AssertionError):
    pass


def _bits(x):
    """float32 values as their uint32 words, -0 taken as +0: fminf / fmaxf and np.minimum / np.maximum may each keep
    either zero of a pair, every other value has one encoding that an exact union can give"""
    return (np.asarray(x, np.float32) + np.float32(0)).view(np.uint32)


def _same(a, b):
    return _bits(a) == _bits(b)


def _first(bad, ids, what, detail=None):
    """raise on the first (lowest) offending id, if any"""
    bad = np.asarray(bad)
    if not bad.any():
        return
    ids = np.asarray(ids)[bad]
    k = int(np.argmin(ids))
    msg = f"{what}: first at {int(ids[k])} ({int(bad.sum())} in all)"
    if detail is not None:
        msg += ": " + detail(np.flatnonzero(bad)[k])
    raise TreeError(msg)


def check_tree(nodes, gid, morton_sorted, aabbs, root_box, max_depth=None, codes=None):
    """Hold a downloaded tree (Scene.bvh_download, Scene.bvh_info) over the AABBs to:
      1. gid is the stable argsort of morton(aabbs) and morton_sorted the codes in that order;
      2. from node 0 every internal node and every leaf is reached exactly once;
      3. a node's leaves are the contiguous run [lo, hi] of sorted positions, hi(left) + 1 == lo(right), the node's own
         index is lo or hi, the root's run is [0, n - 1];
      4. the split is Karras's: with gamma = hi(left), keys gamma and gamma + 1 share exactly as many leading bits as
         keys lo and hi, and an internal left child is node gamma, an internal right child node gamma + 1;
      5. every stored child box is the exact float32 union of that child's subtree (a leaf: its AABB), and root_box is
         the union of the root's two, which is also aabbs' min / max;
      6. max_depth (if given) is the number of levels walked, at most 64.
    Floats are compared bit for bit, with -0 taken as +0 (_bits). The key words are not examined.
    `codes` replaces morton(aabbs) (a refit keeps the build's order: pass the codes of the AABBs the tree was built over).
    Raises TreeError naming the first offending node; returns lo, hi, gamma per node and the level count."""
    aabbs = np.ascontiguousarray(aabbs, np.float32)
    n = aabbs.shape[0]
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
    gid = np.asarray(gid, np.uint32)
    morton_sorted = np.asarray(morton_sorted, np.uint32)
    root_box = np.asarray(root_box, np.float32)
    if n < 1 or nodes.shape[0] != n - 1 or gid.shape != (n,) or morton_sorted.shape != (n,) or root_box.shape != (6,):
        raise TreeError(f"shapes: n {n}, nodes {nodes.shape}, gid {gid.shape}, morton {morton_sorted.shape}")
    want_root = np.concatenate([aabbs[:, :3].min(0), aabbs[:, 3:].max(0)])
    if n == 1:  # the root is the leaf
        if gid[0] != 0 or morton_sorted[0] != 0:
            raise TreeError(f"one leaf: gid {gid[0]}, morton {morton_sorted[0]}")
        if not _same(root_box, want_root).all():
            raise TreeError(f"root box {root_box} is not the leaf's AABB {want_root}")
        if max_depth is not None and max_depth != 1:
            raise TreeError(f"max_depth {max_depth}, one level walked")
        z = np.zeros(0, np.int64)
        return {"lo": z, "hi": z, "gamma": z, "levels": 1}

    # 1. the sort
    if codes is None:
        codes = morton(aabbs)
    order = np.argsort(codes, kind="stable")
    at = np.arange(n)
    _first(gid != order, at, "gid is not the stable argsort of the Morton codes; sorted position",
           lambda k: f"gid {gid[k]}, want {order[k]}")
    _first(morton_sorted != codes[order], at, "morton is not the sorted codes; sorted position",
           lambda k: f"{morton_sorted[k]:#x}, want {codes[order][k]:#x}")

    # 2. every node and leaf referenced once, and all of them reached from node 0
    ref = nodes[:, [L_REF, R_REF]]
    leaf = (ref & LEAF) != 0
    idx = (ref & ~np.uint32(LEAF)).astype(np.int64)
    ni = n - 1
    me = np.arange(ni)
    limit = np.where(leaf, n, ni)
    _first((idx >= limit).any(1), me, "a child reference is out of range; node",
           lambda k: f"refs {ref[k, 0]:#x} {ref[k, 1]:#x}")
    node_refs = np.bincount(idx[~leaf], minlength=ni)
    leaf_refs = np.bincount(idx[leaf], minlength=n)
    if node_refs[0] != 0:
        raise TreeError(f"node 0 (the root) is the child of {me[((idx == 0) & ~leaf).any(1)][0]}")
    _first(node_refs[1:] != 1, me[1:], "internal node not referenced exactly once; node",
           lambda k: f"{node_refs[1 + k]} references")
    _first(leaf_refs != 1, np.arange(n), "leaf not referenced exactly once; Gaussian",
           lambda k: f"{leaf_refs[k]} references")
    levels = []  # the internal nodes of each level; no node is referenced twice, so the walk cannot come back
    frontier = np.zeros(1, np.int64)
    reached = 0
    while frontier.size:
        levels.append(frontier)
        reached += frontier.size
        sub = idx[frontier]
        frontier = sub[~leaf[frontier]]
    if reached != ni:
        seen = np.zeros(ni, bool)
        seen[np.concatenate(levels)] = True
        _first(~seen, me, f"{ni - reached} internal nodes are not reached from node 0; node")
    n_levels = len(levels) + 1  # the deepest internal level's leaves are one level further down

    # 3.-5. from the deepest level to the root: leaf runs, splits, boxes
    pos = np.empty(n, np.int64)
    pos[gid] = at
    keys = sort_keys(morton_sorted)
    fl = nodes.view(np.float32)
    stored = (fl[:, L_BOX], fl[:, R_BOX])
    lo = np.full(ni, -1, np.int64)
    hi = np.full(ni, -1, np.int64)
    gamma = np.full(ni, -1, np.int64)
    box = np.empty((ni, 6), np.float32)
    for lv in reversed(levels):
        run, want = [], []
        for side in (0, 1):
            c, is_leaf = idx[lv, side], leaf[lv, side]
            cn, cl = np.where(is_leaf, 0, c), np.where(is_leaf, c, 0)
            p = pos[cl]
            run.append((np.where(is_leaf, p, lo[cn]), np.where(is_leaf, p, hi[cn])))
            want.append(np.where(is_leaf[:, None], aabbs[cl], box[cn]))
        (llo, lhi), (rlo, rhi) = run
        _first(lhi + 1 != rlo, lv, "the children's leaf runs do not adjoin (hi(left) + 1 != lo(right)); node",
               lambda k: f"left [{llo[k]}, {lhi[k]}], right [{rlo[k]}, {rhi[k]}]")
        _first((lv != llo) & (lv != rhi), lv, "a node's index is not an end of its leaf run; node",
               lambda k: f"run [{llo[k]}, {rhi[k]}]")
        lo[lv], hi[lv], gamma[lv] = llo, rhi, lhi
        want_prefix = clz64(keys[llo] ^ keys[rhi])
        got_prefix = clz64(keys[lhi] ^ keys[lhi + 1])
        _first(got_prefix != want_prefix, lv, "the split is not Karras's; node",
               lambda k: f"run [{llo[k]}, {rhi[k]}] split after {lhi[k]}: keys {lhi[k]} and {lhi[k] + 1} share "
                         f"{got_prefix[k]} bits, the run's ends {want_prefix[k]}")
        for side, want_idx, name in ((0, lhi, "left"), (1, lhi + 1, "right")):
            _first(~leaf[lv, side] & (idx[lv, side] != want_idx), lv,
                   f"an internal {name} child is not node gamma{' + 1' if side else ''}; node",
                   lambda k: f"child {idx[lv[k], side]}, gamma {lhi[k]}")
        for side, name in ((0, "left"), (1, "right")):
            got = stored[side][lv]
            _first(~_same(got, want[side]).all(1), lv, f"the {name} child's box is not the exact union of its subtree; node",
                   lambda k: f"stored {got[k]}, union {want[side][k]}")
        box[lv] = np.concatenate([np.minimum(want[0][:, :3], want[1][:, :3]),
                                  np.maximum(want[0][:, 3:], want[1][:, 3:])], axis=1)
    if lo[0] != 0 or hi[0] != n - 1:
        raise TreeError(f"node 0 (the root) covers [{lo[0]}, {hi[0]}], not [0, {n - 1}]")
    if not _same(root_box, box[0]).all():
        raise TreeError(f"node 0: the root box {root_box} is not the union of the root's children {box[0]}")
    if not _same(root_box, want_root).all():
        raise TreeError(f"node 0: the root box {root_box} is not the AABBs' min / max {want_root}")

    # 6. depth
    if max_depth is not None:
        if max_depth != n_levels:
            raise TreeError(f"max_depth {max_depth}, but {n_levels} levels walked (deepest internal node "
                            f"{int(levels[-1].min())})")
        if max_depth > 64:
            raise TreeError(f"max_depth {max_depth} > 64 (deepest internal node {int(levels[-1].min())})")
    return {"lo": lo, "hi": hi, "gamma": gamma, "levels": n_levels}
