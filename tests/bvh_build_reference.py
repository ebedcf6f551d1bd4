"""The tree pt_bvh_build_device (csrc/pt_bvh_build.hip) must return, restated in numpy from the rules of DESIGN.md §10 and
include/pt_api.h — with other algorithms than the kernels', so that a shared misreading cannot hide:

  Morton order   centroid (hi + lo) * 0.5f; bounds = plain min / max over all centroids; per axis t = (c - lo) / ext (0 where
                 the extent is 0), * 2^21, clamped to [0, 2^21 - 1], truncated — every step in float32; the bits interleaved
                 one at a time, x highest (no magic masks); ordered by np.lexsort on (id, code) (no radix sort)
  LBVH           top-down: the node over sorted positions [first, last] cuts where the highest differing bit of the virtual
                 keys {code, position} changes, found by a linear scan (no per-node binary searches, no parent links);
                 leaf of sorted position i at slot i, the inner node cut at g has its children at inner indices g and g + 1,
                 inner index k at slot n + k, root at slot n
  SAH            top-down: prefix / suffix boxes of the node's range by np.minimum/maximum.accumulate (no range tree), cost
                 area(l) * float32(nl) + area(r) * float32(nr) in float32 in that operand order, the smallest (cost bits,
                 position) wins (a sort, no atomics, no wave reduction); depth + ceil(log2 cnt) >= max_depth -> median cut;
                 post-order layout: the subtree of [first, end) owns slots [base, base + 2 cnt - 1), root last
  boxes          the union of the node's range, taken in one go over the sorted leaf boxes
  depth          leaves count 1, by recursion

The device build keeps fp32 denormals, contracts nothing and divides with correct rounding, so every float here is the
device's bit for bit and the comparison needs no tolerance: `left`, `right`, `prim`, root and depth are compared exactly, boxes
with np.array_equal on the float VALUES.  The one thing left open is the sign of a zero: min / max of -0 and +0 may keep
either on the device (fminf / fmaxf do not order them) and numpy's choice is its own, so a box coordinate that is zero may
differ in its sign bit — that is not part of the contract and -0 == +0 under np.array_equal."""
import numpy as np

from pathtracer_cuda_interactive_amd.host import NODE_DTYPE

LBVH, SAH = 0, 1              # PT_BVH_DEVICE_LBVH, PT_BVH_DEVICE_SAH
GRID = np.float32(2097152.0)  # 2^21 cells per axis
F32 = np.float32


def centroid_codes(lo, hi):
    """63-bit Morton code of every box's centroid, uint64."""
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    c = (hi + lo) * F32(0.5)
    clo, chi = c.min(axis=0), c.max(axis=0)
    ext = chi - clo
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ext > 0, (c - clo) / ext, F32(0)).astype(F32)
    t = np.minimum(np.maximum(t * GRID, F32(0)), F32(2097151.0))
    q = t.astype(np.uint64)                                      # truncation
    codes = np.zeros(len(lo), np.uint64)
    for b in range(21):
        for axis in range(3):                                    # x lands on the highest bit of each triple
            bit = (q[:, axis] >> np.uint64(b)) & np.uint64(1)
            codes |= bit << np.uint64(3 * b + 2 - axis)
    return codes


def morton_order(lo, hi):
    """(primitive ids in Morton order, their codes): by code, equal codes by id."""
    codes = centroid_codes(lo, hi)
    order = np.lexsort((np.arange(len(codes)), codes))
    return order, codes[order]


def _ceil_log2(x):
    return (int(x) - 1).bit_length()


def sah_max_depth(n):
    return min(48, max(8, _ceil_log2(n) + 5))


def lbvh_cut(codes, first, last):
    """Last sorted position of the left child of the node over [first, last] (inclusive, first < last)."""
    if codes[first] != codes[last]:                              # the keys ascend: first and last differ highest
        field = codes[first:last + 1]
        top = (int(codes[first]) ^ int(codes[last])).bit_length() - 1
    else:                                                        # one code: the position half of the virtual key decides
        field = np.arange(first, last + 1, dtype=np.uint64)
        top = (first ^ last).bit_length() - 1
    bit = (field >> np.uint64(top)) & np.uint64(1)               # 0 ... 0 1 ... 1 along the range
    return first + int(np.argmax(bit)) - 1                       # linear scan to where that bit turns 1


def _area(blo, bhi):
    d = np.maximum(bhi - blo, F32(0))
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return F32(2) * (dx * dy + dy * dz + dx * dz)


def sah_cut(slo, shi, first, end, depth, max_depth):
    """First sorted position of the right child of the node over [first, end) at `depth` (root: 1); slo / shi: SORTED leaf boxes."""
    cnt = end - first
    if depth + _ceil_log2(cnt) >= max_depth:
        return first + cnt // 2
    with np.errstate(over="ignore", invalid="ignore"):
        plo, phi = np.minimum.accumulate(slo[first:end]), np.maximum.accumulate(shi[first:end])
        qlo, qhi = np.minimum.accumulate(slo[first:end][::-1])[::-1], np.maximum.accumulate(shi[first:end][::-1])[::-1]
        pos = np.arange(first + 1, end)                          # cut in front of pos: left [first, pos), right [pos, end)
        cost = _area(plo[:-1], phi[:-1]) * (pos - first).astype(F32) + _area(qlo[1:], qhi[1:]) * (end - pos).astype(F32)
    cost = np.ascontiguousarray(cost, F32)
    return int(pos[np.lexsort((pos, cost.view(np.uint32)))[0]])


def build_reference(lo, hi, method):
    """(nodes in NODE_DTYPE, root, depth) of the device builder's tree over the primitive boxes lo, hi (N x 3 float32)."""
    lo, hi = np.ascontiguousarray(lo, F32), np.ascontiguousarray(hi, F32)
    n = len(lo)
    nodes = np.zeros(2 * n - 1, NODE_DTYPE)
    order, codes = morton_order(lo, hi)
    slo, shi = lo[order], hi[order]

    def leaf(slot, i):
        nodes[slot] = (slo[i], shi[i], -1, -1, order[i])
        return 1

    def inner(slot, first, end, left, right):
        nodes[slot] = (slo[first:end].min(axis=0), shi[first:end].max(axis=0), left, right, -1)

    if n == 1:
        leaf(0, 0)
        return nodes, 0, 1

    if method == LBVH:
        def lbvh(first, last, index):                            # -> (slot, depth)
            if first == last:
                return first, leaf(first, first)
            g = lbvh_cut(codes, first, last)
            (l, dl), (r, dr) = lbvh(first, g, g), lbvh(g + 1, last, g + 1)
            inner(n + index, first, last + 1, l, r)
            return n + index, 1 + max(dl, dr)
        root, depth = lbvh(0, n - 1, 0)
    elif method == SAH:
        max_depth = sah_max_depth(n)

        def sah(first, end, base, level):
            cnt = end - first
            if cnt == 1:
                return base, leaf(base, first)
            m = sah_cut(slo, shi, first, end, level, max_depth)
            (l, dl), (r, dr) = sah(first, m, base, level + 1), sah(m, end, base + 2 * (m - first) - 1, level + 1)
            slot = base + 2 * cnt - 2
            inner(slot, first, end, l, r)
            return slot, 1 + max(dl, dr)
        root, depth = sah(0, n, 0, 1)
    else:
        raise ValueError(method)
    return nodes, root, depth


def inorder_prims(nodes, root):
    """Primitive ids of the leaves, left to right."""
    out, stack = [], [int(root)]
    left, right, prim = nodes["left"].tolist(), nodes["right"].tolist(), nodes["prim"].tolist()
    while stack:
        k = stack.pop()
        if prim[k] >= 0:
            out.append(prim[k])
        else:
            stack.append(right[k])
            stack.append(left[k])
    return np.array(out)


def assert_same_tree(want, got, what=""):
    """(nodes, root, depth) twice: ints, root and depth exactly, boxes by value; names the first differing slot."""
    (a, ra, da), (b, rb, db) = want, got
    assert len(a) == len(b), f"{what}: {len(a)} reference nodes, {len(b)} device nodes"
    same = (a["left"] == b["left"]) & (a["right"] == b["right"]) & (a["prim"] == b["prim"])
    same &= (a["bmin"] == b["bmin"]).all(axis=1) & (a["bmax"] == b["bmax"]).all(axis=1)
    if not same.all():
        bad = np.flatnonzero(~same)
        raise AssertionError(f"{what}: {len(bad)} of {len(a)} nodes differ; first at {bad[0]}: reference {a[bad[0]]} device {b[bad[0]]}")
    assert (ra, da) == (rb, db), f"{what}: reference (root, depth) {(ra, da)}, device {(rb, db)}"
