"""Pure-numpy restatement of the reference's `post_processing` (dataloaders/utils.py:193-204) on a VOLUME, for the tests: flood
fills over an explicit stack, no scipy and no skimage (postprocess_ref.py is the same for a plane).
tools/gen_postprocess3d_goldens.py asserts that it equals the reference's function at every voxel of the g22 fixture.

  fill     a background voxel is a hole when no path of 6-neighbour (face) steps through background leads from it to a face of
           the volume (scipy.ndimage.binary_fill_holes, default structure); F = P | holes
  label    the components of F under 26-connectivity (skimage.measure.label's default for a 3-D array)
  filter   total = |F|; component c goes when den * |c| < num * total (the reference: |c| / total < 0.2, i.e. 1 / 5)
  largest  only the largest component of F stays -- among equal sizes the one whose smallest voxel index (z * H + y) * W + x is
           smallest --, after the filter: a volume the filter emptied stays empty

The floods walk a flat copy of the volume with a rim of non-members around it, so no step needs a bounds check.
"""
import numpy as np


def _offsets(shape, faces_only):
    """flat offsets of the 6 or the 26 neighbours in an array of `shape`"""
    _, H, W = shape
    return [(dz * H + dy) * W + dx for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (abs(dz) + abs(dy) + abs(dx) == 1 if faces_only else (dz, dy, dx) != (0, 0, 0))]


def _flood(todo, seed, offs):
    """Clears in `todo` (flat bytearray, 1 = member not reached yet) everything reachable from `seed`; returns what it reached."""
    todo[seed] = 0
    stack, got = [seed], []
    while stack:
        i = stack.pop()
        got.append(i)
        for o in offs:
            if todo[i + o]:
                todo[i + o] = 0
                stack.append(i + o)
    return got


def fill(volume):
    p = np.asarray(volume) != 0
    bg = np.pad(np.pad(~p, 1, constant_values=True), 1, constant_values=False)     # one layer of outside, then the rim
    todo = bytearray(bg.astype(np.uint8).tobytes())
    _flood(todo, int(np.ravel_multi_index((1, 1, 1), bg.shape)), _offsets(bg.shape, True))
    holes = np.frombuffer(bytes(todo), np.uint8).reshape(bg.shape)[2:-2, 2:-2, 2:-2] != 0
    return p | holes


def components(f):
    """-> list of flat voxel index arrays (z * H + y) * W + x, one per 26-connected component of the bool volume f, ordered by
    their smallest index"""
    q = np.pad(np.asarray(f, bool), 1, constant_values=False)
    todo = bytearray(q.astype(np.uint8).tobytes())
    offs = _offsets(q.shape, False)
    out = []
    for seed in np.flatnonzero(q):
        if todo[seed]:
            z, y, x = np.unravel_index(np.array(_flood(todo, int(seed), offs)), q.shape)
            out.append(np.sort(np.ravel_multi_index((z - 1, y - 1, x - 1), f.shape)))
    return out


def select(f, comps, share=(1, 5), largest=False):
    """The filter and the largest-only rule on the filled volume f whose components are `comps` (= components(f); a test that
    runs one volume under several rules labels it once)."""
    out, total = f.copy().reshape(-1), int(f.sum())
    if share is not None:
        for c in comps:
            if share[1] * len(c) < share[0] * total:
                out[c] = False
    if largest and comps:
        sizes = [len(c) for c in comps]
        keep = sizes.index(max(sizes))                     # the first of the largest: components are ordered by smallest index
        for k, c in enumerate(comps):
            if k != keep:
                out[c] = False
    return out.reshape(f.shape)


def process(volume, fill_holes=True, share=(1, 5), largest=False):
    """One volume [D,H,W] -> bool volume.  share = (num, den), or None to keep every component."""
    f = fill(volume) if fill_holes else np.asarray(volume) != 0
    if (share is None or share[0] == 0) and not largest:
        return f
    return select(f, components(f), share, largest)


def volumes(pred, by_class=False, K=1):
    """The binary volumes [N,K,D,H,W] (bool) the entry points read: a class map [N,D,H,W] whose part c is (x == c + 1), or
    volumes [N,(K,)D,H,W] binarised as x != 0."""
    pred = np.asarray(pred)
    if by_class:
        return np.stack([pred.astype(np.int64) == c + 1 for c in range(K)], 1)
    if pred.ndim == 4:
        pred = pred[:, None]
    return pred != 0


def process_batch(pred, by_class=False, K=1, fill_holes=True, share=(1, 5), largest=False):
    """`process` on every volume of `volumes(...)` -> float32 [N,K,D,H,W], what ustrun.functional.post_process_3d returns."""
    p = volumes(pred, by_class, K)
    return np.stack([np.stack([process(q, fill_holes, share, largest) for q in s]) for s in p]).astype(np.float32)


def load_golden(path):
    """tests/golden/g22_postprocess3d.npz -> list of (input [n,D,H,W] bool, the reference's output [n,D,H,W] bool), one per size"""
    z = np.load(path)
    groups = []
    for n, D, H, W in z["sizes"]:
        unpack = lambda a: np.unpackbits(a)[:n * D * H * W].reshape(n, D, H, W).astype(bool)
        groups.append((unpack(z["in_%dx%dx%d" % (D, H, W)]), unpack(z["out_%dx%dx%d" % (D, H, W)])))
    return groups
