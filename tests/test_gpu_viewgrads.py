"""view_color_grads_kernel (csrc/view_grads.hip) alone, against the float64
reference of tests/viewgrads_ref.py: `_C.view_color_grads` and
`_C.view_color_grads_chunked` on synthetic DC rows, no rasterizer involved.

Every case: outputs pre-filled with NaN (an unwritten element fails); the DC
row bit-equal to the float32 sum of the gathered rows in view order; every
other element within 4 * C_KIND * 2^-24 * S of rebuild(float64), S the
element's magnitude sum_v |term_v| (viewgrads_ref's docstring); rows past the
active degrees exactly 0.0.

The bar is sized by the float32 restatement, never by the kernel: C_KIND is
the worst |rebuild(float32) - rebuild(float64)| / (2^-24 S) over the input
families below (tests/test_viewgrads_ref.py measures it again on the CPU):

    kind           measured   C_KIND   bar (4 C_KIND, in units of 2^-24 S)
    sh               9.44       9.5      38
    sg_axis        166.0      167       668
    sg_sharpness   165.4      166       664
    sg_color       168.7      169       676

(the SG kinds' worst element is a lobe with sharpness near 30 and |a| near 1.5
looked at from behind: expf turns the rounding of a . d - 1 into ~150 ulp of g).

Worst kernel error on an MI355X over all cases of this file, in the same units
(helpers.record_margins writes them per case): sh 9.44 (deg_sh3_16_sg7_9),
sg_axis 166.0, sg_sharpness 165.4, sg_color 167.0 (all chunk_P1000_1000) — the
restatement's own figures to three digits (the kernel's arithmetic is the
restatement's), a quarter of the bar.
"""
import functools

import numpy as np
import pytest
import torch

import helpers as Hh
import viewgrads_ref as VR

pytestmark = pytest.mark.gpu


def _C():
    from diff_gaussian_rasterization import _C as C
    return C


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda")  # (a copy: the shared inputs are read-only)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


@functools.lru_cache(maxsize=None)
def _family(name):
    """(family, inputs, float64 reference, S) — computed once per family, shared by the tests, never written."""
    fam, inp = VR.family_inputs(name)
    ref, S = VR.family_rebuild(name, np.float64)
    for a in (*inp.values(), *ref.values(), *S.values()):
        a.setflags(write=False)
    return fam, inp, ref, S


def _run(fam, inp, chunk=0, split=False, misalign=False):
    """The kernel's four outputs (numpy float32) through `_C.view_color_grads` (chunk 0) or
    `_C.view_color_grads_chunked`; `split`: the (dL_dsh DC rows, dL_dsh_rest) layout, joined again here;
    `misalign`: dL_dsh a contiguous view one float into a larger buffer."""
    P, n, SHM, SGM = fam["P"], fam["n_views"], fam["SHM"], fam["SGM"]
    means = _dev(inp["means3D"])
    sg_in = [_dev(inp[k]) for k in ("sg_axis", "sg_sharpness", "sg_color")] if fam["sg_degree"] else [None] * 3
    sg_out = [_nan(P, SGM, 3), _nan(P, SGM), _nan(P, SGM, 3)] if SGM else [None] * 3
    rest = None
    if split:
        dsh, rest = _nan(P, 1, 3), _nan(P, SHM - 1, 3)
    elif misalign:
        dsh = _nan(P * SHM * 3 + 1)[1:].view(P, SHM, 3)
        assert dsh.is_contiguous() and dsh.data_ptr() % 16 == 4
    else:
        dsh = _nan(P, SHM, 3)
        assert dsh.data_ptr() % 16 == 0
    if chunk:
        gathered, cam4 = VR.pack_chunked(inp["rows"], inp["campos"], chunk)
        kw = {"dL_dsh_rest": rest} if split else {}
        _C().view_color_grads_chunked(_dev(gathered), _dev(cam4), n, chunk, means, fam["sh_degree"], dsh,
                                      fam["sg_degree"], *sg_in, *sg_out, **kw)
    else:
        assert not split
        _C().view_color_grads(_dev(VR.pack_flat(inp["rows"], inp["campos"])), n, means, fam["sh_degree"], dsh,
                              fam["sg_degree"], *sg_in, *sg_out)
    torch.cuda.synchronize()
    sh = torch.cat([dsh, rest], 1) if split else dsh
    z = lambda *s: np.zeros(s, dtype=np.float32)  # noqa: E731
    return {"sh": sh.cpu().numpy(),
            "sg_axis": sg_out[0].cpu().numpy() if SGM else z(P, 0, 3),
            "sg_sharpness": sg_out[1].cpu().numpy() if SGM else z(P, 0),
            "sg_color": sg_out[2].cpu().numpy() if SGM else z(P, 0, 3)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_bit_equal(a, b, what, rows=None):
    for kind in VR.KINDS:
        x, y = (a[kind], b[kind]) if rows is None else (a[kind][rows], b[kind][rows])
        assert np.array_equal(_bits(x), _bits(y)), (what, kind, int((_bits(x) != _bits(y)).sum()))


def _check(fam, inp, ref, S, out, what, skip=None):
    """The assertions of every case (module docstring); `skip`: a Gaussian whose non-DC rows are not checked."""
    n, sgd = (fam["sh_degree"] + 1) ** 2, min(fam["sg_degree"], fam["SGM"], VR.MAX_SG)
    keep = np.ones(fam["P"], dtype=bool)
    if skip is not None:
        keep[skip] = False
    want_dc = VR.dc_sum_f32(inp["rows"])
    assert np.array_equal(_bits(out["sh"][:, 0]), _bits(want_dc)), (what, "DC row is not the float32 view-order sum")
    fields = {}
    for kind in VR.KINDS:
        got = out[kind].astype(np.float64)[keep]
        if not got.size:
            continue
        err, bar, s = np.abs(got - ref[kind][keep]), VR.bar(kind, S[kind][keep]), S[kind][keep]
        live = s > 0.0
        worst = float((err[live] / (VR.U * s[live])).max()) if live.any() else 0.0
        print(f"[viewgrads] {what} {kind}: worst {worst:.2f} u S against {4 * VR.C_KIND[kind]:.0f}")
        if live.any():
            fields[kind] = (worst, 4 * VR.C_KIND[kind])
        bad = ~(err <= bar)  # (a NaN — an unwritten element — is bad)
        assert not bad.any(), (what, kind, int(bad.sum()), np.argwhere(bad)[:4].tolist(), worst)
    assert np.all(out["sh"][keep][:, n:] == 0.0), (what, "SH rows past the degree")
    for kind in VR.KINDS[1:]:
        assert np.all(out[kind][keep][:, sgd:] == 0.0), (what, kind, "lobes past the degree")
    Hh.record_margins(fields, what)


# ---- degrees and widths ---------------------------------------------------
@pytest.mark.parametrize("sg", VR.SG_CASES, ids=lambda c: f"sg{c[0]}_{c[1]}")
@pytest.mark.parametrize("sh", VR.SH_CASES, ids=lambda c: f"sh{c[0]}_{c[1]}")
def test_degrees_and_widths(sh, sg):
    """(sh_degree, SHM) x (sg_degree, SGM): SHM < 16 takes the scalar stores, SHM = 17 the e >= 48 zero-fill;
    (0, 3) has null sg_* inputs and all-zero SG outputs; (7, 9) has SGM > kMaxSG, lobes 7 and 8 zero."""
    name = f"deg_sh{sh[0]}_{sh[1]}_sg{sg[0]}_{sg[1]}"
    fam, inp, ref, S = _family(name)
    out = _run(fam, inp)
    _check(fam, inp, ref, S, out, name)
    if sg == (0, 3):
        assert all(out[k].shape[1] == 3 and not out[k].any() for k in VR.KINDS[1:])
    # the chunked entry point on the same rows: the layout must not change a value
    _assert_bit_equal(_run(fam, inp, chunk=128), out, name + " chunked")


def test_misaligned_sh_rows_take_the_scalar_path():
    """SHM = 16 with dL_dsh starting one float into a buffer: sh_rows_vec4 is false, the rows are stored
    element by element, and every value is the aligned run's."""
    fam, inp, ref, S = _family("misaligned")
    out = _run(fam, inp, misalign=True)
    _check(fam, inp, ref, S, out, "misaligned")
    _assert_bit_equal(out, _run(fam, inp), "misaligned against aligned")
    _assert_bit_equal(_run(fam, inp, chunk=128, misalign=True), out, "misaligned, chunked")


# ---- P at block edges -------------------------------------------------------
@pytest.mark.parametrize("P", VR.P_EDGES)
def test_P_at_block_edges(P):
    fam, inp, ref, S = _family(f"P{P}")
    out = _run(fam, inp)
    _check(fam, inp, ref, S, out, f"P{P}")
    _assert_bit_equal(_run(fam, inp, chunk=256), out, f"P{P} chunked")


def test_no_gaussians_is_a_no_op():
    """P = 0 with SH 3 + SG 7 shapes: both entry points return without a launch (nothing to write)."""
    fam = dict(P=0, n_views=3, sh_degree=3, SHM=16, sg_degree=7, SGM=7)
    inp = VR.make_inputs(0, 3, 7, seed=1)
    for chunk in (0, 256):
        out = _run(fam, inp, chunk=chunk)
        assert out["sh"].shape == (0, 16, 3) and out["sg_sharpness"].shape == (0, 7)
    out = _run(fam, inp, chunk=256, split=True)
    assert out["sh"].shape == (0, 16, 3)


# ---- views ------------------------------------------------------------------
@pytest.mark.parametrize("name", [f"views{n}" for n in VR.VIEW_COUNTS] + ["views16_sharp"])
def test_view_counts(name):
    """1, 2, 8 and 16 views; views16_sharp (sharpness 30 on every lobe) is the family the tolerance was meant
    to be sized on."""
    fam, inp, ref, S = _family(name)
    out = _run(fam, inp)
    _check(fam, inp, ref, S, out, name)
    _assert_bit_equal(_run(fam, inp, chunk=77), out, name + " chunked")


def test_views_are_summed_in_view_order():
    """Two views with different rows swapped: the float32 DC sum follows each order exactly (the two orders'
    sums differ in some elements, so a kernel summing in another order fails one of them), and every other
    element changes only within rounding."""
    fam, inp, ref, S = _family("views_swapped")
    swapped = dict(inp)
    swapped["rows"] = inp["rows"][[2, 1, 0]]
    swapped["campos"] = inp["campos"][[2, 1, 0]]
    differ = _bits(VR.dc_sum_f32(inp["rows"])) != _bits(VR.dc_sum_f32(swapped["rows"]))
    assert differ.sum() > 10  # (the inputs do tell the two orders apart)
    ref2, S2 = VR.family_rebuild("views_swapped", np.float64, inp=swapped)
    a, b = _run(fam, inp), _run(fam, swapped)
    _check(fam, inp, ref, S, a, "views in order")
    _check(fam, swapped, ref2, S2, b, "views swapped")
    assert np.array_equal(_bits(a["sh"][:, 0]) != _bits(b["sh"][:, 0]), differ)
    for kind in VR.KINDS:
        err = np.abs(a[kind].astype(np.float64) - b[kind].astype(np.float64))
        assert np.all(err <= VR.bar(kind, S[kind]) + VR.bar(kind, S2[kind])), kind
    _assert_bit_equal(_run(fam, swapped, chunk=128), b, "swapped, chunked")


# ---- the chunked layout -------------------------------------------------------
@pytest.mark.parametrize("P,chunk", VR.CHUNK_CASES)
def test_chunked_layout(P, chunk):
    """Ranges of `chunk` Gaussians: a last range of 1 (513, 256), no short range (512, 256), chunk > P
    (100, 256), chunk = 1, a chunk that is no multiple of anything (7), P - 1, P, P + 1.  Against the float64
    reference, and bit for bit against the unchunked entry point on the same rows."""
    name = f"chunk_P{P}_{chunk}"
    fam, inp, ref, S = _family(name)
    out = _run(fam, inp, chunk=chunk)
    _check(fam, inp, ref, S, out, name)
    _assert_bit_equal(out, _run(fam, inp), name + " against unchunked")


# ---- the split SH layout ------------------------------------------------------
@pytest.mark.parametrize("SHM", [2, 4, 16, 17])
def test_split_sh_layout(SHM):
    """dL_dsh the DC rows [P, 1, 3], dL_dsh_rest the other SHM - 1 (view_color_grads_chunked is the entry point
    that accepts it): bit-equal to the joint layout's rows."""
    fam, inp, ref, S = _family(f"split_{SHM}")
    for chunk in (128, 300):
        out = _run(fam, inp, chunk=chunk, split=True)
        _check(fam, inp, ref, S, out, f"split_{SHM} chunk {chunk}")
        _assert_bit_equal(out, _run(fam, inp, chunk=chunk), f"split_{SHM} against joint")
    _assert_bit_equal(out, _run(fam, inp), f"split_{SHM} against unchunked")


def test_split_sh_layout_needs_two_rows():
    fam, inp, _, _ = _family("split_2")
    P, n = fam["P"], fam["n_views"]
    gathered, cam4 = VR.pack_chunked(inp["rows"], inp["campos"], 128)
    dsh, rest = _nan(P, 1, 3), _nan(P, 0, 3)
    with pytest.raises(RuntimeError, match="split SH layout needs SHM >= 2"):
        _C().view_color_grads_chunked(_dev(gathered), _dev(cam4), n, 128, _dev(inp["means3D"]), 0, dsh,
                                      dL_dsh_rest=rest)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dsh).all())


# ---- isolation ----------------------------------------------------------------
def test_gaussian_at_a_camera_centre_stays_isolated():
    """One Gaussian exactly at view 1's camera centre (|mean - campos| = 0): its own non-DC rows may be NaN,
    its DC row is still the exact sum, and every other Gaussian's rows are bit-equal to a run without it."""
    fam, inp, ref, S = _family("isolation")
    j = 137
    at = {k: v.copy() for k, v in inp.items()}
    at["means3D"][j] = at["campos"][1]
    base = _run(fam, inp)
    _check(fam, inp, ref, S, base, "isolation, base")
    others = np.arange(fam["P"]) != j
    for chunk in (0, 128):
        out = _run(fam, at, chunk=chunk)
        _assert_bit_equal(out, base, f"isolation chunk {chunk}", rows=others)
        _check(fam, at, ref, S, out, f"isolation chunk {chunk}", skip=j)  # (DC row of j included)


# ---- argument guards ------------------------------------------------------------
def _guard_args(SHM=16, SGM=7, P=64, n=3, cpu=False):
    inp = VR.make_inputs(P, n, SGM, seed=9)
    put = (lambda a: torch.from_numpy(np.array(a, order="C"))) if cpu else _dev
    nan = (lambda *s: torch.full(s, float("nan"))) if cpu else _nan
    gathered, cam4 = VR.pack_chunked(inp["rows"], inp["campos"], 32)
    a = dict(flat=put(VR.pack_flat(inp["rows"], inp["campos"])), gathered=put(gathered), campos=put(cam4),
             means3D=put(inp["means3D"]), sg=[put(inp[k]) for k in ("sg_axis", "sg_sharpness", "sg_color")],
             dsh=nan(P, SHM, 3), sgo=[nan(P, SGM, 3), nan(P, SGM), nan(P, SGM, 3)], n=n, chunk=32)
    return a


def _call(a, chunked, sh_degree=3, sg_degree=7):
    if chunked:
        _C().view_color_grads_chunked(a["gathered"], a["campos"], a["n"], a["chunk"], a["means3D"], sh_degree,
                                      a["dsh"], sg_degree, *a["sg"], *a["sgo"])
    else:
        _C().view_color_grads(a["flat"], a["n"], a["means3D"], sh_degree, a["dsh"], sg_degree, *a["sg"], *a["sgo"])


@pytest.mark.parametrize("chunked", [False, True], ids=["flat", "chunked"])
def test_argument_guards(chunked):
    """Each bad call raises RuntimeError and launches nothing (the NaN-filled outputs stay NaN); the two
    wrappers refuse the same things, with the same messages."""
    who = "view_color_grads_chunked" if chunked else "view_color_grads"

    def refused(a, match, **kw):
        with pytest.raises(RuntimeError, match=match):
            _call(a, chunked, **kw)
        if a["dsh"].is_cuda:
            torch.cuda.synchronize()
        for t in (a["dsh"], *a["sgo"]):
            assert bool(torch.isnan(t).all()), match

    a = _guard_args()
    _call(a, chunked)  # (the arguments themselves are good)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a["dsh"]).all())

    a = _guard_args()  # wrong `gathered` length
    a["flat"], a["gathered"] = a["flat"][:-1], a["gathered"][:-1]
    refused(a, f"{who}: `gathered` must hold")
    if chunked:
        a = _guard_args()
        a["chunk"] = 0
        refused(a, "chunk >= 1")
    a = _guard_args()  # no views
    a["n"], a["flat"], a["gathered"], a["campos"] = 0, a["flat"][:0], a["gathered"][:0], a["campos"][:0]
    refused(a, "invalid arguments")
    a = _guard_args(SGM=3)  # sg_degree > SGM
    refused(a, f"{who}: degrees \\(SH 3, SG 7\\) do not fit 16 SH rows and 3 SG lobes")
    a = _guard_args(SHM=25)  # sh_degree = 4
    refused(a, f"{who}: degrees \\(SH 4, SG 7\\) do not fit 25 SH rows and 7 SG lobes", sh_degree=4)
    a = _guard_args(SHM=9)  # SHM < (sh_degree + 1)^2
    refused(a, f"{who}: degrees \\(SH 3, SG 7\\) do not fit 9 SH rows and 7 SG lobes")
    a = _guard_args(cpu=True)  # host tensors
    refused(a, f"{who}: `\\w+` must be a contiguous fp32 HIP tensor")
    a = _guard_args()  # a non-contiguous dL_dsh
    a["dsh"] = _nan(64, 16, 6)[:, :, :3]
    refused(a, f"{who}: `dL_dsh` must be a contiguous fp32 HIP tensor")
    a = _guard_args()  # an SG output missing
    a["sgo"][0] = None
    with pytest.raises(RuntimeError, match=f"{who}: `dL_dsg_axis` must be a contiguous fp32 HIP tensor"):
        _call(a, chunked)
