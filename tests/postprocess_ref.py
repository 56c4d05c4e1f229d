"""Pure-numpy restatement of the reference's `post_processing` (dataloaders/utils.py:193-204) for the tests: flood fills over an
explicit stack, no scipy and no skimage.  tools/gen_postprocess_goldens.py asserts that it equals the reference's function at every
pixel of the g18 fixture.

  fill    a background pixel is a hole when no path of 4-neighbour (cross) steps through background leads from it to the image
          border (scipy.ndimage.binary_fill_holes, default structure); F = P | holes
  label   the components of F under 8-connectivity (skimage.measure.label's default for a plane)
  filter  total = |F|; component c goes when den * |c| < num * total (the reference: |c| / total < 0.2, i.e. 1 / 5)
"""
import numpy as np

N4 = ((0, -1), (0, 1), (-1, 0), (1, 0))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def _flood(member, seen, seeds, nbrs):
    """Marks in `seen` everything reachable from `seeds` through `member`; returns the pixels reached."""
    H, W = member.shape
    stack, got = [], []
    for y, x in seeds:
        if member[y, x] and not seen[y, x]:
            seen[y, x] = True
            stack.append((y, x))
    while stack:
        y, x = stack.pop()
        got.append((y, x))
        for dy, dx in nbrs:
            v, u = y + dy, x + dx
            if 0 <= v < H and 0 <= u < W and member[v, u] and not seen[v, u]:
                seen[v, u] = True
                stack.append((v, u))
    return got


def fill(plane):
    p = np.asarray(plane) != 0
    H, W = p.shape
    rim = [(y, x) for y in range(H) for x in ((0, W - 1) if 0 < y < H - 1 else range(W))]
    outside = np.zeros((H, W), bool)
    _flood(~p, outside, rim, N4)
    return ~outside


def components(f):
    """-> list of pixel lists, one per 8-connected component of the bool plane f"""
    seen = np.zeros(f.shape, bool)
    return [_flood(f, seen, [(y, x)], N8) for y, x in zip(*np.nonzero(f)) if not seen[y, x]]


def process(plane, fill_holes=True, share=(1, 5)):
    """One 2-D plane -> bool plane.  share = (num, den), or None to keep every component."""
    f = fill(plane) if fill_holes else np.asarray(plane) != 0
    if share is None or share[0] == 0:
        return f
    out, total = f.copy(), int(f.sum())
    for c in components(f):
        if share[1] * len(c) < share[0] * total:
            ys, xs = zip(*c)
            out[list(ys), list(xs)] = False
    return out


def planes(pred, by_class=False, K=1):
    """The binary planes [N,K,H,W] (bool) the entry points read: a class map [N,H,W] whose part c is (x == c + 1), or planes
    [N,(K,)H,W] binarised as x != 0."""
    pred = np.asarray(pred)
    if by_class:
        return np.stack([pred.astype(np.int64) == c + 1 for c in range(K)], 1)
    if pred.ndim == 3:
        pred = pred[:, None]
    return pred != 0


def process_batch(pred, by_class=False, K=1, fill_holes=True, share=(1, 5)):
    """`process` on every plane of `planes(...)` -> float32 [N,K,H,W], what ustrun.functional.post_process returns."""
    p = planes(pred, by_class, K)
    return np.stack([np.stack([process(q, fill_holes, share) for q in s]) for s in p]).astype(np.float32)


def load_golden(path):
    """tests/golden/g18_postprocess.npz -> list of (input [n,H,W] bool, the reference's output [n,H,W] bool), one per size"""
    z = np.load(path)
    groups = []
    for n, H, W in z["sizes"]:
        unpack = lambda a: np.unpackbits(a)[:n * H * W].reshape(n, H, W).astype(bool)
        groups.append((unpack(z["in_%dx%d" % (H, W)]), unpack(z["out_%dx%d" % (H, W)])))
    return groups
