"""float64 reference for tests that plant inf / NaN: every element of an expected result is classified as finite, +inf, -inf or
NaN, and finite elements carry their value after rounding to the storage type.

The expected result is computed with torch float64 operators on the CPU from the inputs AS STORED (`stored`: `.half()` /
`.bfloat16()` first, then `.double()`) and rounded to the storage type with torch's own cast (`expect`).  The classes do not depend
on the summation order as long as no finite partial sum can overflow float64 or the kernel's f32 accumulator: the callers keep to
small integers plus a handful of planted values.

Two ReLU conventions: "torch" propagates NaN (relu(nan) = nan, relu'(nan) passes the gradient); "select" is `x > 0 ? x : 0` with the
backward mask `a > 0 ? g : 0` (what fmaxf / v_med3 / a compare-and-select give: NaN -> 0)."""
import torch

FINITE, PINF, NINF, NAN = 0, 1, 2, 3
CLASS_NAMES = ("finite", "+inf", "-inf", "nan")
STORAGE = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
CONVENTIONS = ("torch", "select")


def stored(x, elt):
    """the value a kernel reads: x rounded to the storage type (overflow -> inf, as Tensor.half() does), as float64"""
    return x.to(STORAGE[elt]).double()


def classify(x):
    """int8 tensor of FINITE / PINF / NINF / NAN, elementwise"""
    x = x.detach()
    c = torch.zeros(x.shape, dtype=torch.int8)
    c[x == float("inf")] = PINF
    c[x == float("-inf")] = NINF
    c[x != x] = NAN
    return c


def expect(ref64, elt):
    """(class, value): the float64 result rounded to the storage type by torch's cast, then classified; `value` is that rounded
    result as float64 (meaningful where class == FINITE)"""
    assert ref64.dtype == torch.float64
    r = ref64.detach().to(STORAGE[elt]).double()
    return classify(r), r


def relu(x, convention="torch"):
    assert convention in CONVENTIONS
    if convention == "torch":
        return torch.relu(x)
    return torch.where(x > 0, x, torch.zeros_like(x))


def relu_bwd(a, g, convention="torch"):
    """gradient of relu at pre-activation `a` (or at the activation itself: the sign test is the same) for upstream g"""
    assert convention in CONVENTIONS
    if convention == "torch":
        return torch.where(a <= 0, torch.zeros_like(g), g)          # NaN fails `<= 0`: the gradient passes
    return torch.where(a > 0, g, torch.zeros_like(g))


def mismatches(got, ref64, elt):
    """Compare a device result (any float dtype, on the CPU) with the float64 expectation: returns (n_class, n_value, text) --
    elements whose class differs, finite-class elements whose bits differ from the storage-rounded value, and a description of the
    first few of either.  No tolerance: class equality, then equality of the rounded values (0.0 == -0.0)."""
    cls, val = expect(ref64, elt)
    g = got.detach().cpu().double()
    assert g.shape == val.shape, (tuple(g.shape), tuple(val.shape))
    gcls = classify(g)
    bad_c = gcls != cls
    bad_v = (cls == FINITE) & (gcls == FINITE) & (g != val)
    lines = []
    for what, bad in (("class", bad_c), ("value", bad_v)):
        for idx in bad.nonzero()[:6].tolist():
            i = tuple(idx)
            lines.append("%s at %s: got %r (%s), expected %r (%s)" % (what, i, float(g[i]), CLASS_NAMES[int(gcls[i])], float(val[i]),
                                                                       CLASS_NAMES[int(cls[i])]))
    return int(bad_c.sum()), int(bad_v.sum()), "; ".join(lines)


def assert_matches(got, ref64, elt, what=""):
    """gates 2 and 3 in one: every element's class equals the reference's, every finite one equals it to the bit"""
    nc, nv, text = mismatches(got, ref64, elt)
    assert nc == 0 and nv == 0, "%s: %d class / %d value mismatches: %s" % (what, nc, nv, text)


def which_convention(got, refs, elt):
    """refs: {"torch": ref64, "select": ref64}.  Returns the names of the conventions the device result matches exactly."""
    return [k for k in CONVENTIONS if k in refs and mismatches(got, refs[k], elt)[:2] == (0, 0)]
