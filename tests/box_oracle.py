"""DESIGN.md S14 in NumPy: per view and label the tight bounding box and the pixel count of an ids tensor -- a plain
restatement with a loop over labels, what the box stage's tensor is compared with bit for bit -- and seeded ids
tensors for it to work on."""
import numpy as np

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def boxes(ids, K, transposed):
    """i32 [views, K, 5]: (xmin, ymin, xmax, ymax, count) of the pixels of `ids` ([views, nslow, nfast]) equal to each
    label 0 ... K-1, (W, H, -1, -1, 0) where there is none.  Storage is [view][y][x], or [view][x][y] if transposed."""
    ids = np.asarray(ids)
    assert ids.ndim == 3 and ids.dtype == np.int32
    views, nslow, nfast = ids.shape
    W, H = (nslow, nfast) if transposed else (nfast, nslow)
    out = np.empty((views, K, 5), np.int32)
    for v in range(views):
        for l in range(K):
            slow, fast = np.nonzero(ids[v] == l)
            if slow.size == 0:
                out[v, l] = (W, H, -1, -1, 0)
                continue
            x, y = (slow, fast) if transposed else (fast, slow)
            out[v, l] = (x.min(), y.min(), x.max(), y.max(), x.size)
    return out


def labels(rng, shape, K):
    """Seeded ids of `shape`: 40 % background, 45 % labels in range, the rest K-1 and ids that belong to no row (K, K + 7,
    -2, INT32_MIN, INT32_MAX).  Label K-1 is present; with K > 1 label min(1, K - 2) is absent, so empty rows occur."""
    n = int(np.prod(shape))
    kind = rng.random(n)
    a = np.full(n, -1, np.int64)
    inr = (kind >= 0.40) & (kind < 0.85)
    a[inr] = rng.integers(0, K, int(inr.sum()))
    top = (kind >= 0.85) & (kind < 0.90)
    a[top] = K - 1
    odd = kind >= 0.90
    a[odd] = rng.choice(np.array([K, K + 7, -2, INT32_MIN, INT32_MAX], np.int64), int(odd.sum()))
    if K > 1:
        absent = min(1, K - 2)
        a[a == absent] = K - 1
    a[rng.integers(0, n)] = K - 1
    return a.astype(np.int32).reshape(shape)
