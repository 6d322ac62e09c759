"""NumPy restatement of the one-pass, recursion-free formulation of the OctoMap .bt records that csrc/r3d_octree.hip runs on
the GPU: a second oracle beside oracle/octomap_ref.write_bt_bytes (which walks the tree recursively).  bt_body(codes) ->
(record bytes, node count) for ascending unique 48-bit Morton codes."""
import numpy as np


def bt_body(codes):
    codes = np.asarray(codes, dtype=np.uint64); n = len(codes)
    if n == 0: return b"", 0
    if n == 8**16: return b"\0\0", 1
    # cpl[i]: number of leading 3-bit digits shared with codes[i-1]; -1 for i == 0 (so the root starts there)
    cpl = np.full(n, -1, np.int64)
    x = codes[1:] ^ codes[:-1]
    hb = np.floor(np.log2(x.astype(np.float64))).astype(np.int64)  # fine for < 2^48 after fixup
    hb = np.where((x >> hb.astype(np.uint64)) == 0, hb - 1, hb); hb = np.where((x >> (hb+1).astype(np.uint64)) != 0, hb + 1, hb)
    cpl[1:] = 15 - hb // 3
    # f[i]: depth of the topmost full subtree holding code i (16 = none)
    f = np.full(n, 16, np.int64)
    idx = np.arange(n)
    for d in range(15, 0, -1):
        sz = 8 ** (16 - d)
        if sz > n: break
        m = np.uint64(sz - 1)
        first = idx - (codes & m).astype(np.int64)          # where the subtree's first code would be
        ok = (first >= 0) & (first + sz <= n)
        fi = np.where(ok, first, 0)
        ok &= (codes[fi] == (codes & ~m)) & (codes[np.minimum(fi + sz - 1, n - 1)] == (codes | m))
        f = np.where(ok, d, f)
    top = np.minimum(15, f - 1)                 # deepest inner depth starting at i
    cnt = np.maximum(0, top - cpl)              # inner nodes starting at i: depths cpl+1 .. top
    base = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    n_inner = int(cnt.sum())
    rec = np.zeros(n_inner, np.uint16)
    n_leaf = 0
    for j in range(n):
        # emitted nodes that start at j, depth e in cpl+1 .. min(16, f): e == 0 is the root (no parent)
        for e in range(max(cpl[j] + 1, 1), min(16, f[j]) + 1):
            inner = e <= 15 and e < f[j]
            n_leaf += not inner
            d = e - 1
            if d > cpl[j]:
                pos = base[j] + (d - cpl[j] - 1)
            else:
                sh = np.uint64(3 * (16 - d))
                j0 = int(np.searchsorted(codes, (codes[j] >> sh) << sh)) if d > 0 else 0
                pos = base[j0] + (d - cpl[j0] - 1)
            digit = int((codes[j] >> np.uint64(3 * (15 - d))) & np.uint64(7))
            rec[pos] |= (3 if inner else 2) << (2 * digit)
    return rec.astype("<u2").tobytes(), n_inner + n_leaf
