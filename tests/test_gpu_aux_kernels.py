"""GPU: the kernels between the convolutions, one at a time through their engine-free entry points (vc_*_host, each calling the launch
function the engine calls), against the references of tests/aux_cases.py (held to their own conditions on the CPU by
tests/test_aux_cases.py).

The SPPF pooling kernels, the nearest upsample, MaxPool2d(3, 2, 1), the layout kernel and the bf16 -> fp8 cast select, copy or round to
nearest even: they are compared with assert_array_equal on values (so -0 equals +0) and there is no tolerance to choose.  Every SPPF case
also asserts which kernel launch_sppf_pool reports to have launched, and with which slice width.  The fused ReID stem is held to the
bf16 conv gate of tests/test_gpu_kernels.py::test_conv2d and, bit for bit, to conv -> NumPy max-pool.  AvgPool + L2 has the one derived
bound (test_avgpool_l2norm)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import aux_cases as A  # noqa: E402
import vehicle_counting_amd.engine as E  # noqa: E402

SPPF_GROUPS = {}
for _c in A.sppf_cases().values():
    SPPF_GROUPS.setdefault("%dx%dx%d-%s-form%d" % (*_c.shape, _c.precision, _c.form), []).append(_c.name)


@pytest.mark.parametrize("group", sorted(SPPF_GROUPS))
def test_sppf_pool(group):
    """One (shape, element type, form), every channel count of the table: the reported kernel and slice width are the ones the case claims
    to cover; the sentinel channels before and after the four slices are untouched, the input slice is unchanged, and the three
    output slices equal the direct 5 x 5 / 9 x 9 / 13 x 13 window maxima."""
    for name in SPPF_GROUPS[group]:
        c = A.sppf_cases()[name]
        buf = c.buffer()
        out, kernel, ws = E.sppf_pool(buf, c.C, c.co, c.precision, c.form)
        assert (kernel, ws) == c.expect, name
        lo, hi = c.co, c.co + 4 * c.C
        np.testing.assert_array_equal(out[..., :lo], buf[..., :lo], err_msg=name + ": channels before the slices")
        np.testing.assert_array_equal(out[..., hi:], buf[..., hi:], err_msg=name + ": channels after the slices")
        np.testing.assert_array_equal(out[..., lo:lo + c.C], buf[..., lo:lo + c.C], err_msg=name + ": input slice")
        ref = A.sppf_ref(name)
        for i, r in enumerate((2, 4, 6)):
            np.testing.assert_array_equal(out[..., lo + (i + 1) * c.C:lo + (i + 2) * c.C], ref[..., i * c.C:(i + 1) * c.C],
                                          err_msg="%s: radius %d (%s, ws %d)" % (name, r, kernel, ws))


@pytest.mark.parametrize("form", [1, 0])
def test_sppf_pool_refuses_a_channel_count_no_kernel_takes(form):
    """bf16 with C = 12: no slice width divides it and the plain kernel works on 8 channels at a time -- VC_ERR_ARG from the launcher's
    argument check, before any launch."""
    buf = np.full((1, 5, 6, 80), A.SENTINEL, np.float32)
    with pytest.raises(E.L.VcError) as ex:
        E.sppf_pool(buf, 12, 16, "bf16", form)
    assert ex.value.code == 1 and "alignment" in str(ex.value)


@pytest.mark.parametrize("precision", A.PRECISIONS)
@pytest.mark.parametrize("shape", A.UPSAMPLE_SHAPES)
def test_upsample2x(shape, precision):
    x = A.upsample_input(shape, precision)
    dst = np.full((shape[0], 2 * shape[1], 2 * shape[2], A.UPSAMPLE_CS), A.SENTINEL, np.float32)
    out = E.upsample2x(x, dst, A.UPSAMPLE_CO, precision)
    lo, hi = A.UPSAMPLE_CO, A.UPSAMPLE_CO + A.UPSAMPLE_C
    np.testing.assert_array_equal(out[..., lo:hi], A.upsample_ref(x))
    assert (out[..., :lo] == A.SENTINEL).all() and (out[..., hi:] == A.SENTINEL).all()


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("shape", A.MAXPOOL_SHAPES)
def test_maxpool3s2(shape, precision):
    """both template instances (the engine only launches the f32 one: the bf16 stem is fused), padding -inf: channel 0 is negative everywhere"""
    x = A.maxpool_input(shape, precision)
    ref = A.maxpool_ref(x)
    dst = np.full((*ref.shape[:3], A.MAXPOOL_CS), A.SENTINEL, np.float32)
    out = E.maxpool3s2(x, dst, A.MAXPOOL_CO, precision)
    lo, hi = A.MAXPOOL_CO, A.MAXPOOL_CO + A.MAXPOOL_C
    np.testing.assert_array_equal(out[..., lo:hi], ref)
    assert (out[..., :lo] == A.SENTINEL).all() and (out[..., hi:] == A.SENTINEL).all()


def test_maxpool3s2_refuses_a_slice_its_vector_stores_cannot_take():
    """the kernel stores 16 bytes at a time: a destination slice that starts at channel 4 of a bf16 buffer is VC_ERR_ARG, not a
    misaligned store (launch_maxpool3s2 checked the strides only)"""
    x = A.maxpool_input((1, 2, 2), "bf16")
    with pytest.raises(E.L.VcError) as ex:
        E.maxpool3s2(x, np.zeros((1, 1, 1, A.MAXPOOL_CS), np.float32), 4, "bf16")
    assert ex.value.code == 1 and "alignment" in str(ex.value)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("shape", A.LAYOUT_SHAPES)
def test_nchw_to_nhwc_pad(shape, precision):
    x = A.layout_input(shape)
    out = E.nchw_to_nhwc_pad(x, precision)
    np.testing.assert_array_equal(out, A.layout_ref(x, precision))
    assert out.shape[-1] == (4 if precision == "f32" else 8) and (out[..., shape[1]:] == 0).all()      # pad channels exactly 0


@pytest.mark.parametrize("inv_scale", A.FP8_INV_SCALES)
def test_bf16_to_fp8_on_every_bf16_value(inv_scale):
    """All 65536 bf16 bit patterns but the NaNs in one launch: saturation at +-448 (the infinities included), ties to even, e4m3
    subnormals and the underflow to zero, against float32 product -> clip -> torch's e4m3fn rounding (tests/test_gpu_fp8.py::q8)."""
    v = A.all_bf16_values()
    src = np.full((len(v), A.FP8_SRC_CS), 7.0, np.float32)
    src[:, A.FP8_SRC_CO:A.FP8_SRC_CO + A.FP8_C] = v
    dst = np.full((len(v), A.FP8_DST_CS), 0x5a, np.uint8)
    out = E.bf16_to_fp8(src, A.FP8_C, A.FP8_SRC_CO, inv_scale, dst, A.FP8_DST_CO)
    lo, hi = A.FP8_DST_CO, A.FP8_DST_CO + A.FP8_C
    assert (out[:, :lo] == 0x5a).all() and (out[:, hi:] == 0x5a).all()
    got, ref = A.e4m3_values(out[:, lo:hi]), A.fp8_cast_ref(v, inv_scale)
    bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    print("inv_scale %r: %d of %d values differ" % (inv_scale, bad.sum(), bad.size))
    for x, g, r in list(zip(v[bad], got[bad], ref[bad]))[:20]:
        print("   bf16 %r (0x%04x) -> device %r, reference %r" % (float(x), int(np.float32(x).view(np.uint32)) >> 16, float(g), float(r)))
    np.testing.assert_array_equal(got, ref)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("k", A.REID_STEM_K)
def test_reid_stem_pool(k):
    """reid_stem_pool_kernel against float64 conv -> ReLU -> bf16 -> MaxPool2d(3, 2, 1) at the bf16 conv gate (test_conv2d's: the max
    adds no rounding), and bit for bit against E.conv2d(precision="bf16") -> NumPy max-pool, as reid_stem.hip's header claims (under the
    tile configuration launch_conv's heuristic picks for this shape).  k = 60: 780 items on a grid of 704, so 76 workgroups run a second
    item whose patch came through the register prefetch; the crops differ, so an item computed from the wrong patch cannot pass."""
    x, w, b = A.reid_stem_input(k)
    y = E.reid_stem_pool(x, w, b)
    ref = A.reid_stem_ref(k)
    assert y.shape == ref.shape == (k, 25, 25, 64)
    err = np.abs(y - ref) - (2e-3 + 2.0 ** -7 * np.abs(ref))
    print("k = %d: worst excess over the gate %.3g (negative = inside), %d of %d outputs differ from the reference's own rounding"
          % (k, err.max(), (y != ref).sum(), y.size))
    np.testing.assert_allclose(y, ref, rtol=2 ** -7, atol=2e-3)
    two = A.pool3s2_nhwc(E.conv2d(x, w, b, stride=1, pad=1, act=2, precision="bf16"))
    print("k = %d: %d of %d outputs differ in bits from conv -> pool" % (k, (_bits(y) != _bits(two)).sum(), y.size))
    np.testing.assert_array_equal(_bits(y), _bits(two))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("case", A.AVGPOOL_CASES)
def test_avgpool_l2norm(case, precision):
    """avgpool_l2norm_kernel against float64 on the same (rounded) inputs, within a derived bound.

    With u = 2^-24 and n = h * w pixels, per crop and channel c the kernel computes
      a^_c = fl(fl(sum_i x_ic) / n): n - 1 sequential adds and one divide, so |a^_c - a_c| <= ((n - 1) u S_c + u |s_c|) / n <= e_c := n u A_c,
        where S_c = sum_i |x_ic|, A_c = S_c / n (the mean magnitude) and a_c the exact mean;
      ss^ = sum_c a^_c^2: one rounded square per term, then a tree of depth 10 (1 add in the thread, 6 wave shuffles, 3 adds of the four
        wave sums); all terms are >= 0, so ss^ = ||a^||^2 (1 + t), |t| <= 11 u;
      nrm^ = fl(sqrt(ss^)) = ||a^|| (1 + t'), |t'| <= 11 u / 2 + u;  out_c = fl(a^_c / nrm^) = (a^_c / ||a^||)(1 + t''), |t''| <= 7.5 u.
    The map a -> a / ||a|| moves by at most (e_c + |y_c| ||e||_2) / ||a|| to first order when a moves by e (y = a / ||a||), hence
      |out_c - y_c| <= (n u A_c + |y_c| n u ||A||_2) / ||a|| + 7.5 u |y_c|
    to first order in u; aux_cases.avgpool_bound multiplies by 1.001 for the second-order terms (n u < 1e-6).  The division, the square
    root and the final divide are taken as correctly rounded (one u each).  tests/test_aux_cases.py asserts the bound stays below the
    network-level gate of 2e-5 on these inputs; the worst observed ratio to the bound is printed and recorded in DESIGN.md section 5."""
    x = A.avgpool_input(case, precision)
    out = E.avgpool_l2norm(x, precision)
    ref, bound = A.avgpool_ref(x), A.avgpool_bound(x)
    assert out.shape == ref.shape == bound.shape and out.dtype == np.float32
    ratio = np.abs(out.astype(np.float64) - ref) / bound
    print("%s %s: worst |error| / bound per crop %s (bound at most %.3g)" % (case, precision, np.round(ratio.max(axis=1), 3).tolist(), bound.max()))
    assert (ratio <= 1.0).all(), ratio.max()
