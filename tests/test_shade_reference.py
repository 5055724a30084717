"""The deferred shade's HIP kernels against the float64 reference (tests/shade_reference.py) on the cases of tests/shade_cases.py, every case x shipped variant.
Exact set: the oracle's bits, so the oracle's statement (tests/test_shade_reference_cpu.py) is the exact set's. Fast set: decision words within the project's
shade cap of the reference's, every unflipped geometry pixel within slack + one R11G11B10 code of float64, and - where slack is below a quarter of a code - within
one code of the oracle, the sentence the parity tests state. The fused upscale + shade launch, the unlit skip and the fast BRDF LUT are held to the same.

The references and the oracle's runs are the CPU module's, computed once per case x variant."""
import numpy as np
import pytest

import parity
import pass_parity as pp
import passes
import shade_cases as sc
import shade_reference as sr
import test_shade_reference_cpu as cpu
from plainrenderer_amd import pixfmt
from test_variants_parity import SHADE_VARIANTS

PAIRS = cpu.PAIRS
FUSED_VARIANTS = sorted({(b, m, aa, n) for b, m, aa, tech, n in SHADE_VARIANTS if tech == 0})   # the fused launch has indirect technique 0 only
FUSED_REFERENCE_VARIANT = (2, 0, True, 3)
SKIP_UNLIT_VARIANTS = [(2, 0, True, 0, 3), (0, 1, False, 0, 3), (1, 2, True, 1, 4), (3, 3, True, 0, 1), (2, 0, False, 1, 2)]  # tests/test_shade_unlit_skip.py's
GI_Y_SH, GI_COCG = (0.03, 0.004, -0.003, 0.002), (0.001, -0.0005)
_ids = lambda v: "-".join(str(int(x)) for x in v) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def noise_idx(backend):
    _, idx = passes.make_bindless(backend, [], 1, sc.case(sc.NAMES[0]).noise)  # the four stand-ins are the same arrays in every case
    return tuple(idx)


@pytest.fixture()
def fast(backend):
    backend.setMathMode(True)
    yield backend
    backend.setMathMode(False)


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", PAIRS, ids=_ids)
def test_gpu_exact_set_is_the_oracle_and_within_the_reference_bound(backend, noise_idx, name, variant):
    c = sc.case(name)
    ref = cpu.reference(name, variant)
    oracle_packed, oracle_words = cpu.oracle_run(name, variant)
    backend.setMathMode(False)
    got = passes.gpu_deferred_shading(backend, *c.args(variant[0], noise_idx), *variant).reshape(c.h, c.w)
    assert np.array_equal(got, oracle_packed), "%d words differ from the oracle's" % int((got != oracle_packed).sum())
    flips, worst, _ = cpu.statement(got, oracle_words, ref)
    assert flips == 0 and worst <= 1.0


_rows = {}


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", PAIRS, ids=_ids)
def test_gpu_fast_set_is_within_slack_and_one_code_of_the_reference(fast, noise_idx, name, variant):
    c = sc.case(name)
    ref = cpu.reference(name, variant)
    oracle_packed, _ = cpu.oracle_run(name, variant)
    with passes.gpu_signature(fast, c.w * c.h) as sg:
        got = passes.gpu_deferred_shading(fast, *c.args(variant[0], noise_idx), *variant).reshape(c.h, c.w)
    pp.fast_only(fast, "shade %s" % name)
    words = (sg.words & 0xff).reshape(c.h, c.w)
    flips, worst, cm = cpu.statement(got, words, ref)
    geo = ~ref.sky
    ok = geo & (words == ref.words)
    d = parity.r11g11b10_code_diff(got, oracle_packed).reshape(c.h, c.w, 3).max(-1)
    slack = cm["slack_codes"].max(-1)
    at = np.unravel_index(np.argmax(np.where(ok, d, -1)), d.shape)
    row = dict(flips=flips, worst=worst, d=int(d[at]), slack_there=float(slack[at]), well_d=int(d[ok & cm["well"]].max(initial=0)))
    if name == "mirror_highlight":
        oracle_excess = sr.compare(oracle_packed, ref)["excess"]
        floor = ok & c.floor_columns
        row.update(floor_d=int(d[floor].max()), floor_fast_excess=float(cm["excess"][floor].max()), floor_oracle_excess=float(oracle_excess[floor].max()),
                   floor_over_one=float((d[floor] > 1).mean()))
    _rows.setdefault(name, []).append(row)
    if len(_rows[name]) == len([p for p in PAIRS if p[0] == name]):
        rows = _rows[name]
        worst_row = max(rows, key=lambda r: r["d"])
        extra = {}
        if name == "mirror_highlight":
            extra = dict(floor_columns_max_code_diff_to_oracle=max(r["floor_d"] for r in rows), floor_columns_share_over_one_code=max(r["floor_over_one"] for r in rows),
                         floor_columns_fast_excess_codes=max(r["floor_fast_excess"] for r in rows), floor_columns_oracle_excess_codes=max(r["floor_oracle_excess"] for r in rows))
        pp.report("shade_ref_fast", case=name, pixels=int(geo.sum()), variants=len(rows), flips=sum(r["flips"] for r in rows), worst_excess_codes=max(r["worst"] for r in rows),
                  max_code_diff_to_oracle=worst_row["d"], slack_codes_there=worst_row["slack_there"], well_conditioned_max_code_diff_to_oracle=max(r["well_d"] for r in rows), **extra)
    assert np.array_equal(words[ref.sky], ref.words[ref.sky]), "sky pixels are marked 128"
    assert flips <= pp.count_cap(2e-3, int(geo.sum())), "%d decision words differ from the reference's" % flips
    assert worst <= 1.0, "the fast set is %.3f codes outside slack + one code of float64" % (worst - 1.0)
    assert d[ok & cm["well"]].max(initial=0) <= 1, "slack below a quarter of a code: every channel within one R11G11B10 code of the oracle"


@pytest.mark.gpu
@pytest.mark.parametrize("variant", FUSED_VARIANTS, ids=_ids)
@pytest.mark.parametrize("name", sc.NAMES)
def test_gpu_fused_launch_equals_the_separate_fast_launches(fast, noise_idx, name, variant):
    """upscale + shade at pass fusion 2, 1 and 0 on constant half-resolution GI images and the G-buffer's own half depth: the same bytes. With that the fused
    launch inherits the statement of the separate shade; for one variant per case it is also held to the reference on the GI texels the upscale wrote."""
    c = sc.case(name)
    brdf, multi, aa, cascades = variant
    tw, th = c.w // 2, c.h // 2
    half_ysh = pixfmt.pack_half(np.broadcast_to(np.asarray(GI_Y_SH, np.float32), (th, tw, 4)))
    half_cocg = pixfmt.pack_half(np.broadcast_to(np.asarray(GI_COCG, np.float32), (th, tw, 2)))
    half_depth = passes.orc_depth_downscale(c.gb["depth"], c.w, c.h)
    common = (c.gb, c.w, c.h, sc.lut(brdf), sc.LUT_RES, c.light, c.shadow_info, c.shadow_maps, sc.SHADOW_RES)
    tail = (c.froxel, c.froxel_dims, c.vol_settings, c.sky, c.global_packed(noise_idx))
    run = lambda **kw: passes.gpu_upscale_and_shade(fast, half_ysh, half_cocg, tw, th, half_depth, *common, *tail, brdf, multi, aa, cascades, **kw)
    assert pp.upscale_is_regular(c.w, c.h)
    try:
        fused = run()
        assert fast.getPassFusion() == (2, 2), "the two executions ran inside one fused launch"
        pp.fast_only(fast, "upscale + shade, fusion 2")
        fast.setPassFusion(1)
        one, y1, c1 = run(download_upscaled=True)
        pp.fast_only(fast, "upscale + shade, fusion 1")
        fast.setPassFusion(0)
        sep, ys, cs = run(download_upscaled=True)
        assert fast.getPassFusion() == (0, 0)
        pp.fast_only(fast, "upscale + shade, fusion 0")
    finally:
        fast.setPassFusion(2)
    assert np.array_equal(fused, sep) and np.array_equal(one, sep), "fusion 2 / 1 / 0: %d / %d words differ" % ((fused != sep).sum(), (one != sep).sum())
    assert np.array_equal(ys, y1) and np.array_equal(cs, c1)
    if variant != FUSED_REFERENCE_VARIANT:
        return
    full = (brdf, multi, aa, 0, cascades)
    args = list(c.args(brdf, noise_idx))
    args[9], args[10] = ys, cs
    alone = passes.gpu_deferred_shading(fast, *args, *full)
    assert np.array_equal(alone, sep), "the shade alone on the upscaled texels"
    ref = sr.shade(*args, c.noise_by_index(noise_idx), *full)
    with passes.gpu_signature(fast, c.w * c.h) as sg:
        signed = run()
    assert np.array_equal(signed, fused)
    words = (sg.words & 0xff).reshape(c.h, c.w)
    flips, worst, _ = cpu.statement(fused.reshape(c.h, c.w), words, ref)
    assert flips <= pp.count_cap(2e-3, int((~ref.sky).sum())) and worst <= 1.0, (flips, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", SKIP_UNLIT_VARIANTS, ids=_ids)
@pytest.mark.parametrize("name", ["grazing_and_terminator", "cascades_and_taps"])
def test_gpu_unlit_skip_changes_no_byte(fast, noise_idx, monkeypatch, name, variant):
    c = sc.case(name)
    args = c.args(variant[0], noise_idx)
    monkeypatch.setenv("PLR_SHADE_SKIP_UNLIT", "0")
    full = passes.gpu_deferred_shading(fast, *args, *variant)
    monkeypatch.delenv("PLR_SHADE_SKIP_UNLIT")
    skipping = passes.gpu_deferred_shading(fast, *args, *variant)
    pp.fast_only(fast, "shade %s" % name)
    assert np.array_equal(full, skipping), "%d words differ between PLR_SHADE_SKIP_UNLIT=0 and the default" % int((full != skipping).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("brdf", [0, 1, 2, 3])
def test_gpu_fast_brdf_lut_against_float64(fast, brdf):
    ref = sr.brdf_lut(sc.LUT_RES, brdf)
    raw, _ = passes.gpu_brdf_lut(fast, sc.LUT_RES, brdf)
    got = pixfmt.unpack_half(raw).reshape(sc.LUT_RES, sc.LUT_RES, 4).astype(np.float64)
    steps = sr.half_steps(got[..., :3], ref[..., :3])
    print("PARITY brdf_lut_fast_f64 brdf=%d res=%d max_steps=%.3f within_half_step=%.5f" % (brdf, sc.LUT_RES, steps.max(), (steps <= 0.5).mean()))
    assert np.isfinite(got).all() and (got[..., 3] == 0).all()
    assert steps.max() <= cpu.ORACLE_LUT_STEPS + 1.0, "the oracle's measured distance plus the one step the fast LUT is allowed against the oracle"
