"""numpy restatement of the two overlay pictures of the reference's utils/util.py (draw_mask_and_save :367-390,
draw_contour_and_save :299-365) in the batch forms ustrun.render takes, and the decoding of tests/golden/g17_render.npz.

  mask_overlay     every step as the reference evaluates it: the range rule in f32 (an add rounded, then a multiply rounded),
                   colour and halving in float64, truncation; the clamp to 0..255 only defines what numpy's cast leaves undefined.
  contour_float    the float image the reference hands to cv2.imwrite: (img - min) / (max - min) * 255 in f32, then the
                   contours (3 x 3 dilation with background outside the image, minus the map) in its drawing order.  A constant
                   image gives 0 here where the reference has 0 / 0 (the one deviation of the device path, restated).
  saturate         cv2's documented saturating cast: round half to even, clamp to 0..255.
  contour_value64  the same value in float64, to find the pixels that sit within 1e-4 of a half-integer (where a one-level
                   difference is allowed: the tests cap their share).
The fixture stores its images as uint16 sources q with a rule per image, so that it stays small: `decode_image`.
"""
import numpy as np

MASK_COLOURS = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255)], dtype=np.float64)
PRED_COLOURS = MASK_COLOURS[1:]          # util.py:348
GT_COLOUR = MASK_COLOURS[0]              # util.py:347


def planes_eq1(pred, parts=None):
    """bool [N,P,H,W]: where a part is ON for the mask overlay (planes: value == 1; labels: label == i + 1)."""
    if pred.dtype == np.int64:
        return np.stack([pred == i + 1 for i in range(parts)], axis=1)
    return pred == 1


def planes_fg(m, parts=None):
    """bool [N,P,H,W]: foreground for the contour overlay (planes: value > 0; labels: label == i + 1)."""
    if m.dtype == np.int64:
        return np.stack([m == i + 1 for i in range(parts)], axis=1)
    return m > 0


def three(img):
    """[C,H,W] -> [H,W,3], one channel repeated"""
    if img.shape[0] == 1:
        img = np.repeat(img, 3, axis=0)
    return img.transpose(1, 2, 0)


def mask_overlay(img, pred, parts=None):
    """img f32 [N,C,H,W]; pred f32 [N,P,H,W] or int64 [N,H,W] with `parts` -> uint8 [N,H,W,3]"""
    assert img.dtype == np.float32
    on = planes_eq1(pred, parts)
    out = []
    for n in range(len(img)):
        x = img[n]
        if x.min() < -0.5:
            v = (x + np.float32(1)) * np.float32(127.5)
        elif x.max() < 1.5:
            v = x * np.float32(255)
        else:
            v = x
        assert v.dtype == np.float32
        v = three(v).astype(np.float64)
        rgb, fac = np.zeros(v.shape), np.ones(v.shape)
        for i in reversed(range(on.shape[1])):
            fac[on[n, i]] = 0.5
            rgb[on[n, i]] = MASK_COLOURS[i]
        out.append(np.clip(np.trunc((v + rgb) * fac), 0, 255).astype(np.uint8))
    return np.stack(out)


def dilate3(b):
    """3 x 3 binary dilation of bool [H,W], background outside the image"""
    p = np.pad(b, 1)
    H, W = b.shape
    d = np.zeros_like(b)
    for dy in range(3):
        for dx in range(3):
            d |= p[dy:dy + H, dx:dx + W]
    return d


def _draw(v, pred, gt, parts):
    fp, fg = planes_fg(pred, parts), planes_fg(gt, parts)
    for n in range(len(v)):
        for i in range(fp.shape[1]):
            v[n][dilate3(fp[n, i]) & ~fp[n, i]] = PRED_COLOURS[i]
            v[n][dilate3(fg[n, i]) & ~fg[n, i]] = GT_COLOUR
    return v


def contour_float(img, pred, gt, parts=None):
    """-> f32 [N,H,W,3]: what the reference passes to cv2.imwrite (as RGB)"""
    assert img.dtype == np.float32
    v = []
    for x in img:
        lo, hi = x.min(), x.max()
        s = (x - lo) / (hi - lo) * np.float32(255) if hi != lo else np.zeros_like(x)
        assert s.dtype == np.float32
        v.append(three(s).copy())
    return _draw(np.stack(v), pred, gt, parts)


def contour_value64(img, pred, gt, parts=None):
    """the same picture with the scaling evaluated in float64 -> f64 [N,H,W,3]"""
    v = []
    for x in img.astype(np.float64):
        lo, hi = x.min(), x.max()
        v.append(three((x - lo) / (hi - lo) * 255.0 if hi != lo else np.zeros_like(x)).copy())
    return _draw(np.stack(v), pred, gt, parts)


def saturate(v):
    """float -> uint8 as cv2's saturate_cast<uchar> is documented: round half to even, clamp"""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def contour_overlay(img, pred, gt, parts=None):
    return saturate(contour_float(img, pred, gt, parts))


def near_half(v64, eps=1e-4):
    """bool: the value lies within eps of a half-integer"""
    return np.abs(v64 - np.floor(v64) - 0.5) < eps


# ---- fixture g17 --------------------------------------------------------------------------------------------------------
# image n of a case = rule[n] applied to its uint16 source: 0 -> [-1, 1], 1 -> [0, 1], 2 -> [0, 256) in steps of 1 / 256
def decode_image(q, rule):
    out = []
    for qn, r in zip(q.astype(np.float32), rule):
        if r == 0:
            out.append(qn / np.float32(32767.5) - np.float32(1))
        elif r == 1:
            out.append(qn / np.float32(65535))
        else:
            out.append(qn / np.float32(256))
    return np.stack(out).astype(np.float32)


def fixture_cases(Z, kind):
    """names of the `kind` ("mask" / "contour") cases"""
    return [str(n) for n in Z["cases_" + kind]]


def fixture_inputs(Z, name):
    """-> (img f32 [N,C,H,W], pred, gt or None, parts): pred / gt f32 planes [N,P,H,W] or int64 labels [N,H,W]"""
    img = decode_image(Z[name + "_q"], Z[name + "_rule"])
    parts = int(Z[name + "_parts"])
    cast = (lambda a: a.astype(np.int64)) if int(Z[name + "_kind"]) == 1 else (lambda a: a.astype(np.float32))
    gt = cast(Z[name + "_gt"]) if name + "_gt" in Z.files else None
    return img, cast(Z[name + "_pred"]), gt, parts
