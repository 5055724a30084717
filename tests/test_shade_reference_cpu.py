"""The oracle's deferred shade against the float64 reference (tests/shade_reference.py) on the cases of tests/shade_cases.py, every case x shipped variant:
equal decision words (the cases' margins leave no decision to a rounding) and |unpack(oracle) - reference| <= slack + one R11G11B10 code at the reference
value, per channel, on every geometry pixel. The cases are well-conditioned where they claim to be; each seeded mistake of the reference makes the same
check fail; the oracle's BRDF LUT is held to the float64 LUT. Nothing here needs a GPU.

Measured on the CPU (profiles/r12_shade_reference.txt): zero flips, and the oracle's largest |difference| - slack is 0.50 codes in every case - its own final
rounding - so the oracle needs no k above K_ULPS = 8 (it needs none at all) and no term had to be added to the perturbation set."""
import numpy as np
import pytest

import pass_parity as pp
import passes
import shade_cases as sc
import shade_reference as sr
from plainrenderer_amd import pixfmt
from test_variants_parity import SHADE_VARIANTS

# Measured on the CPU: 1.096 steps, at ONE texel (r = 1 / 32, NoV = 0.1 / 32, the Fresnel-weighted and the plain sum: 6.4e-4 and 5.1e-4 of the value); every other
# texel of the four LUTs is within 0.52 steps, the half step of the final rounding. The expectation from 1024 fp32 additions was at most one step, and the sums are
# not what misses it: at that texel V grazes the surface and L.z = 2 (V.H) H.z - V.z cancels to the last bits for the samples near the horizon, where
# Vis * VoH * NoL / NoH is largest (NoV = 0.003 and NoL -> 0 under the 0.5 / (v1 + v2)) and `NoL > 0` decides whether a sample counts at all.
ORACLE_LUT_STEPS = 1.1
# fp32 roundings of the mode-0 lobe where every 1 - energy is >= 1 / 8, in half-ulps (2^-24) of the lobe, each counted at its worst: the energy fit's eight
# roundings reach 1 - energyAverage eightfold (64), the LUT fetch's four reach 1 - energyIncoming eightfold (32), 1 - energyOutgoing (1), the unscaled lobe's
# products and division (5), fresnelAverage (3), its square times the energy (2 + 8), the scaling's denominator >= 0.4 (25), the last product (1): 141 -> 160.
# pi for 3.1415 moves the lobe by 2.9e-5 = 495 of these units.
MULTISCATTER_KAT_HALF_ULPS = 160
WELL_SHARE = 0.95

_refs = {}
_oracle = {}


def reference(name, variant):
    """computed once per case x variant, shared, never written to"""
    if (name, variant) not in _refs:
        _refs[name, variant] = sc.case(name).reference(variant)
    return _refs[name, variant]


def oracle_run(name, variant):
    if (name, variant) not in _oracle:
        import pyoracle as orc
        c = sc.case(name)
        arr = (orc.OrcImage * 4)()
        keep = [orc.Img(np.ascontiguousarray(t), 32, 32, passes.F.RG8) for t in c.noise]
        for i, im in enumerate(keep):
            arr[i] = im.c
        with passes.orc_signature(c.w * c.h) as so:
            out = passes.orc_deferred_shading(*c.args(variant[0]), arr, 4, *variant)
        _oracle[name, variant] = (out.reshape(c.h, c.w), so.words.reshape(c.h, c.w).copy())
    return _oracle[name, variant]


def statement(packed, words, ref):
    """-> (flips, worst excess in codes over the unflipped geometry pixels, compare()'s dict): the statement is flips == 0 (or the cap) and excess <= 1"""
    cm = sr.compare(packed, ref)
    flips = words != ref.words
    ok = ~ref.sky & ~flips
    worst = float(cm["excess"][ok].max()) if ok.any() else 0.0
    if not cm["finite"][ok].all():
        worst = float("inf")
    return int(flips.sum()), worst, cm


_worst = {}


# a variant that cannot be finite on a case is not run on it (shade_cases.NOT_FINITE, with the reason)
PAIRS = [(name, variant) for name in sc.NAMES for variant in SHADE_VARIANTS if (name, variant) not in sc.NOT_FINITE]


@pytest.mark.parametrize("name,variant", PAIRS, ids=lambda v: "-".join(str(int(x)) for x in v) if isinstance(v, tuple) else str(v))
def test_oracle_is_within_slack_and_one_code_of_the_reference(oracle, name, variant):
    c = sc.case(name)
    ref = reference(name, variant)
    c.check(ref, variant)
    packed, words = oracle_run(name, variant)
    flips, worst, cm = statement(packed, words, ref)
    geo = ~ref.sky
    region = geo & c.well_columns if name == "mirror_highlight" else geo
    well = float(cm["well"][region].mean())
    _worst.setdefault(name, []).append((worst, well, flips, float(cm["slack_codes"][geo].max())))
    if len(_worst[name]) == len([p for p in PAIRS if p[0] == name]):
        rows = _worst[name]
        pp.report("shade_ref_oracle", case=name, pixels=int(geo.sum()), variants=len(rows), flips=sum(r[2] for r in rows), worst_excess_codes=max(r[0] for r in rows),
                  least_well_conditioned_share=min(r[1] for r in rows), largest_slack_codes=max(r[3] for r in rows))
    assert np.array_equal(words[ref.sky], ref.words[ref.sky]) and flips == 0, "%d decision words differ" % flips
    assert worst <= 1.0, "the oracle is %.3f codes outside slack + one code" % (worst - 1.0)
    assert well >= WELL_SHARE, "slack is below a quarter of a code on only %.4f of the pixels" % well


# a case x variant on which each seeded mistake must show (the first that does is enough; all are tried in this order)
CATCHES = {
    "roughness_floor": [("mirror_highlight", (2, 0, False, 0, 3)), ("material_lattice", (2, 0, True, 0, 3))],
    "schlick_exponent": [("material_lattice", (2, 0, True, 0, 3))],
    "srgb_knee": [("material_lattice", (2, 0, True, 0, 3))],
    "nov_floor": [("grazing_and_terminator", (2, 0, False, 1, 2)), ("grazing_and_terminator", (2, 0, True, 0, 3))],
    "pcf_compare": [("cascades_and_taps", (2, 0, True, 0, 3))],
    "cascade_compare": [("cascades_and_taps", (2, 0, True, 0, 3))],
    "froxel_linear_z": [("fog_and_indirect", (2, 0, True, 0, 3))],
}


def multiscattering_kat(pi_of_mode_0=None):
    """The oracle's computeSpecularMultiscatteringLobe in mode 0 (its KAT entry point) against the reference's: roughness codes 0 .. 255, NoL from 0 to 1, f0 of
    dielectrics and metals, the LUT texel at (r, NoV = 0.6) - where the lobe is well-conditioned: 1 - energyIncoming, 1 - energyOutgoing and 1 - energyAverage
    all >= 1 / 8 (each is a difference from one; behind 1 / 8 an absolute half-ulp of the energy is at most 8 half-ulps of the factor).
    -> the largest |oracle - reference| / reference in units of 2^-24"""
    import pyoracle as orc
    lut_u16 = sc.lut(2)
    lut = pixfmt.unpack_half(lut_u16).reshape(sc.LUT_RES, sc.LUT_RES, 4).astype(np.float64)
    f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
    codes, nol, f0 = np.meshgrid(np.arange(256), np.linspace(0.0, 1.0, 17), [0.04, 0.3, 0.97], indexing="ij")
    r = f32(np.maximum((codes.reshape(-1) / 255.0) ** 2, 0.0045))
    nol = f32(nol.reshape(-1))
    f0 = f32(f0.reshape(-1, 1) * np.array([1.0, 0.9, 0.7]))
    texel = f32(sr.sample_linear_2d(lut, r, np.full(r.size, 0.6)))[:, :3]
    single = f32(0.1 + f0)
    keep = ((1.0 - sr.sample_linear_2d(lut, r, nol)[:, 1] >= 0.125) & (1.0 - texel[:, 1] >= 0.125) & (1.0 - sr.reflected_energy_average(r) >= 0.125))
    assert keep.sum() >= 2000 and len(np.unique(r[keep])) >= 100, keep.sum()
    r, nol, f0, texel, single = r[keep], nol[keep], f0[keep], texel[keep], single[keep]
    got = orc.kat_specular_multiscattering(orc.Img(lut_u16, sc.LUT_RES, sc.LUT_RES, passes.F.RGBA16_sFloat), 0, np.concatenate([r[:, None], nol[:, None], f0, single, texel], 1))
    kw = {} if pi_of_mode_0 is None else {"pi_of_mode_0": pi_of_mode_0}
    want = sr.specular_multiscattering_lobe(0, lut, r, nol, f0, single, texel, **kw)
    assert np.isfinite(want).all() and (want > 0).all()
    return float((np.abs(got.astype(np.float64) - want) / want).max() * 2.0 ** 24)


def test_oracle_multiscattering_lobe_against_float64(oracle):
    err = multiscattering_kat()
    print("PARITY shade_ref_multiscatter_kat mode=0 max_rel_err_in_half_ulps=%.2f" % err)
    assert err <= MULTISCATTER_KAT_HALF_ULPS


@pytest.mark.parametrize("mistake", sr.MISTAKES)
def test_the_reference_can_fail(oracle, mistake):
    """each seeded mistake makes the oracle-against-reference check fail on at least one case"""
    if mistake == "multiscatter_pi":
        # 2.9e-5 of one lobe: a three-hundredth of an R11G11B10 code, so no colour image can show it (measured: the worst excess of every case stays at 0.50 codes
        # with the mistake seeded). The case that catches it is the lobe itself, held to the oracle's in fp32 ulps
        err = multiscattering_kat(pi_of_mode_0=sr.PI)
        print("MISTAKE %-18s caught by the multiscattering lobe's KAT: max_rel_err_in_half_ulps=%.1f (bound %d)" % (mistake, err, MULTISCATTER_KAT_HALF_ULPS))
        assert err > MULTISCATTER_KAT_HALF_ULPS
        return
    seen = []
    for name, variant in CATCHES[mistake]:
        wrong = sc.case(name).reference(variant, mistake=mistake)
        packed, words = oracle_run(name, variant)
        flips, worst, _ = statement(packed, words, wrong)
        seen.append("%s: flips %d, worst excess %.3f codes" % (name, flips, worst))
        if flips > 0 or worst > 1.0:
            print("MISTAKE %-18s caught by %s %s: flips=%d worst_excess_codes=%.3f" % (mistake, name, variant, flips, worst))
            return
    pytest.fail("no case catches the seeded mistake %r (%s)" % (mistake, "; ".join(seen)))


@pytest.mark.parametrize("brdf", [0, 1, 2, 3])
def test_oracle_brdf_lut_against_float64(oracle, brdf):
    ref = sr.brdf_lut(sc.LUT_RES, brdf)
    got = pixfmt.unpack_half(passes.orc_brdf_lut(sc.LUT_RES, brdf)).reshape(sc.LUT_RES, sc.LUT_RES, 4).astype(np.float64)
    assert np.isfinite(ref).all() and (got[..., 3] == 0).all()
    steps = sr.half_steps(got[..., :3], ref[..., :3])
    print("PARITY brdf_lut_oracle_f64 brdf=%d res=%d max_steps=%.3f within_half_step=%.5f" % (brdf, sc.LUT_RES, steps.max(), (steps <= 0.5).mean()))
    assert steps.max() <= ORACLE_LUT_STEPS
