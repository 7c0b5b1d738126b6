"""A from-scratch reference of what a BVH refit has to leave behind (tests/test_refit.py): the
leaf records, the float child boxes and the 64-byte quantized nodes, from nothing but the
triangles' vertices and the tree's topology (child words, leaf order). numpy only; nothing here
calls the product.

Layouts (csrc/common/yrt_gpu_types.h, yrt_qnode.h): a float node is 128 B: lox[4] hix[4] loy[4]
hiy[4] loz[4] hiz[4], child[4], 16 B padding; a child word is (index << 5) | count, count > 0 a
leaf of `count` records from leaf slot `index`, count 0 the inner node `index`, -1 empty. A leaf
record is 48 B: v0 xyz + triangle id, e1 xyz + flags, e2 xyz + geometry id. A quantized node is
64 B: origin xyz, the three biased exponents, child[4], six words of plane bytes (lo x, hi x,
lo y, hi y, lo z, hi z; byte k = child k), 8 B padding.
"""
import numpy as np

F = np.float32


# ----------------------------------------------------------------------------- the exports, taken apart
def split_nodes(nodes):
    """(planes (n, 6, 4) float32: lox hix loy hiy loz hiz per child, children (n, 4) int32,
    padding (n, 16) uint8) of exported float nodes."""
    nd = np.asarray(nodes, np.uint8).reshape(-1, 128)
    return (nd[:, :96].copy().view(F).reshape(-1, 6, 4), nd[:, 96:112].copy().view(np.int32),
            nd[:, 112:].copy())


def split_tris(tris, tri_bytes=48):
    """(v0, e1, e2 (m, 3) float32, w (m, 3) int32: triangle id, flags, geometry id) of exported
    leaf records, in leaf order."""
    rec = np.asarray(tris, np.uint8).reshape(-1, tri_bytes)[:, :48].copy().view(F).reshape(-1, 3, 4)
    return rec[:, 0, :3], rec[:, 1, :3], rec[:, 2, :3], rec[:, :, 3].copy().view(np.int32)


# ----------------------------------------------------------------------------- leaf records
def leaf_records(tri9, gid):
    """Per leaf slot (gid: the slot's triangle id) v0, e1 = v0 - v1, e2 = v2 - v0 in float32."""
    t = np.ascontiguousarray(tri9, F)[np.asarray(gid)]
    return t[:, 0:3], t[:, 0:3] - t[:, 3:6], t[:, 6:9] - t[:, 0:3]


# ----------------------------------------------------------------------------- float boxes
def union_boxes(children, gid, tri9):
    """The child boxes bottom-up: a leaf child's box is the min / max of its triangles' nine
    vertices, an inner child's the union of that node's valid child boxes. min and max are exact,
    so no order matters. Returns (planes (n, 6, 4) float32 in the node layout, 0 in empty slots;
    valid (n, 4))."""
    children = np.asarray(children, np.int32)
    v = np.ascontiguousarray(tri9, F).reshape(-1, 3, 3)
    tlo, thi = v.min(1), v.max(1)
    n = len(children)
    lo = np.zeros((n, 4, 3), F)
    hi = np.zeros((n, 4, 3), F)
    valid = children != -1
    order, seen = [0], {0}
    for ni in order:                                   # parents before children
        for c in children[ni][valid[ni]]:
            if c & 31 == 0:
                assert (c >> 5) not in seen, "a node with two parents"
                seen.add(int(c >> 5))
                order.append(int(c >> 5))
    assert len(order) == n, "unreachable nodes"
    for ni in reversed(order):
        for k in np.flatnonzero(valid[ni]):
            idx, cnt = int(children[ni, k]) >> 5, int(children[ni, k]) & 31
            if cnt:
                g = np.asarray(gid)[idx:idx + cnt]
                lo[ni, k], hi[ni, k] = tlo[g].min(0), thi[g].max(0)
            else:
                assert valid[idx].any(), "an inner node without children"
                lo[ni, k], hi[ni, k] = lo[idx][valid[idx]].min(0), hi[idx][valid[idx]].max(0)
    planes = np.zeros((n, 6, 4), F)
    planes[:, 0::2, :] = lo.transpose(0, 2, 1)
    planes[:, 1::2, :] = hi.transpose(0, 2, 1)
    return planes, valid


# ----------------------------------------------------------------------------- quantized nodes
def _float_down(d):
    """The largest float32 <= d (float64, finite, within the float range)."""
    f = d.astype(F)
    return np.where(f.astype(np.float64) > d, np.nextafter(f, F(-np.inf)), f).astype(F)


def quantize(planes, children):
    """The 64-byte quantized nodes of float nodes, from the definition in yrt_qnode.h's header
    comment, in float64 and integers. Per node and axis, over the valid children:
      quantum 2^e: the smallest power of two >= extent / 250 and >= 2^(floor(log2 m) - 22), m the
        largest |coordinate|, e clamped to [-126, 127] (-126 when extent and m are 0);
      origin: the largest float <= lo_min - 2 * 2^e;
      q_lo = floor((lo - origin) / 2^e) - 1, q_hi = ceil((hi - origin) / 2^e) + 1, kept in
        [0, 255]; empty slots 255 / 0; an axis without children: origin 0, exponent 127.
    Returns uint8 (n * 64,)."""
    P = np.asarray(planes, F).astype(np.float64)
    children = np.asarray(children, np.int32)
    n = len(children)
    valid = children != -1
    some = valid.any(1)
    v3 = valid[:, None, :]
    lo, hi = P[:, 0::2, :], P[:, 1::2, :]                                   # (n, 3, 4)
    L = np.where(v3, lo, np.inf).min(2)
    H = np.where(v3, hi, -np.inf).max(2)
    L, H = np.where(some[:, None], L, 0.0), np.where(some[:, None], H, 0.0)

    def ceil_log2(x):                 # the smallest e with 2^e >= x, x > 0: x = m * 2^k, m in [0.5, 1)
        m, k = np.frexp(x)
        return np.where(m == 0.5, k - 1, k)

    ext = H - L
    e = np.full((n, 3), -126, np.int64)
    pos = ext > 0
    e[pos] = ceil_log2(ext[pos] / 250.0)
    big = np.maximum(np.abs(L), np.abs(H))
    nz = big > 0
    floor_log2 = np.frexp(big[nz])[1] - 1
    e[nz] = np.maximum(e[nz], floor_log2 - 22)
    e = np.clip(e, -126, 127)
    s = np.ldexp(1.0, e)
    origin = _float_down(L - 2.0 * s)
    o = origin.astype(np.float64)
    qlo = np.floor((lo - o[:, :, None]) / s[:, :, None]) - 1
    qhi = np.ceil((hi - o[:, :, None]) / s[:, :, None]) + 1
    qlo = np.where(v3, np.clip(qlo, 0, None), 255).astype(np.int64)
    qhi = np.where(v3, np.clip(qhi, None, 255), 0).astype(np.int64)
    assert ((qlo >= 0) & (qlo <= 255) & (qhi >= 0) & (qhi <= 255)).all()
    origin = np.where(some[:, None], origin, F(0))
    ebias = np.where(some[:, None], e + 127, 127).astype(np.uint32)

    out = np.zeros((n, 64), np.uint8)
    out[:, 0:12] = np.ascontiguousarray(origin, F).view(np.uint8)
    exps = ebias[:, 0] | (ebias[:, 1] << 8) | (ebias[:, 2] << 16)
    out[:, 12:16] = np.ascontiguousarray(exps, np.uint32).view(np.uint8).reshape(n, 4)
    out[:, 16:32] = np.ascontiguousarray(children).view(np.uint8)
    q = np.empty((n, 6, 4), np.uint8)                 # word = plane, byte k = child k (little endian)
    q[:, 0::2, :] = qlo
    q[:, 1::2, :] = qhi
    out[:, 32:56] = q.reshape(n, 24)
    return out.reshape(-1)
