"""The tests' own anisotropic reference (tests/prepass_aniso_reference.py): the probe count by hand at the exact boundaries n^2 rmin == rmax, the round-half-even
quotient by hand, a run with A <= 1 against the isotropic references bit for bit on their existing cases, the input conditions of the GPU cases
(tests/prepass_aniso_cases.py), and the entry point and the header at the C boundary; no GPU."""
import os

import numpy as np
import pytest

import prepass_aniso_cases as an
import prepass_aniso_reference as aniso
import prepass_bc_cases as bc
import prepass_normal_cases as nc
import prepass_texture_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_probe_count_by_hand_at_the_exact_boundaries():
    """N is the smallest integer in [1, A] with !(N N rmin < rmax): at rmax == n^2 rmin exactly the comparison is false and N = n; one ulp above it N = n + 1"""
    for A in (2, 5, 8, 16):
        for n in range(1, 17):
            for rmin in (1.0, 0.375, 3.0, 2.0 ** -40):
                rmax = float(n * n) * rmin  # exact: n^2 <= 256 has 9 bits, these rmin at most 2
                assert int(aniso.probe_count(rmin, rmax, A)) == min(n, A), (A, n, rmin)
                assert int(aniso.probe_count(rmin, np.nextafter(rmax, np.inf), A)) == min(n + 1, A), (A, n, rmin)
                if n > 1:
                    assert int(aniso.probe_count(rmin, np.nextafter(rmax, 0.0), A)) == min(n, A)
    # by hand: rmin 1, rmax 9.0625 (the major_x case): 1 < 9.0625, 4 < 9.0625, 9 < 9.0625, 16 >= 9.0625: N = 4 - and with rmin 1.25: 11.25 >= 9.0625: N = 3
    assert int(aniso.probe_count(1.0, 9.0625, 8)) == 4 and int(aniso.probe_count(1.25, 9.0625, 8)) == 3
    assert int(aniso.probe_count(1.0, 9.0625, 2)) == 2 and int(aniso.probe_count(1.0, 9.0625, 3)) == 3


def test_probe_count_of_the_degenerate_footprints():
    assert int(aniso.probe_count(0.0, 1.0, 8)) == 8, "rmin = 0 < rmax: N = A"
    assert int(aniso.probe_count(0.0, 0.0, 8)) == 1, "rmax = 0: N = 1"
    assert int(aniso.probe_count(np.nan, 1.0, 8)) == 1 and int(aniso.probe_count(1.0, np.nan, 8)) == 1, "a NaN compares false: N = 1"
    assert int(aniso.probe_count(1.0, np.inf, 16)) == 16 and int(aniso.probe_count(np.inf, np.inf, 16)) == 1
    assert aniso.probe_count(np.array([1.0, 1.0, 0.0]), np.array([1.0, 4.5, 0.0]), 8).tolist() == [1, 3, 1]


def test_stored_code_is_the_quotient_rounded_half_to_even_by_hand():
    """code = T / (N 2^24) rounded half to even; for N = 1 it is the sampling contract's (S + 2^23 - 1 + ((S >> 24) & 1)) >> 24"""
    q = lambda T, N: int(aniso.round_half_even_quotient(np.int64(T), np.int64(N << 24))[0])
    for N in (1, 2, 3, 5, 6, 7, 16):
        D = N << 24
        assert q(0, N) == 0 and q(255 * D, N) == 255
        assert q(10 * D + D // 2, N) == 10 and q(11 * D + D // 2, N) == 12, "exactly a half: to the even code"
        assert q(10 * D + D // 2 + 1, N) == 11 and q(11 * D + D // 2 - 1, N) == 11
    rng = np.random.default_rng(1)
    S = rng.integers(0, (255 << 24) + 1, 4096, dtype=np.int64)
    S[:512] = (S[:512] >> 24 << 24) | (1 << 23)  # halves
    got = aniso.round_half_even_quotient(S, np.int64(1 << 24))[0]
    assert np.array_equal(got, (S + (1 << 23) - 1 + ((S >> 24) & 1)) >> 24)


@pytest.mark.parametrize("A", [0, 1])
@pytest.mark.parametrize("name", list(tc.CASES))
def test_without_anisotropy_the_reference_is_the_texture_reference(oracle, name, A):
    for case, tex, r, s in tc.reference(name):
        got = aniso.sample(case, tex, r["keys"], A)
        assert np.array_equal(got["albedo"], s["albedo"]) and np.array_equal(got["specular"], s["specular"])


@pytest.mark.parametrize("name", list(bc.CASES))
def test_without_anisotropy_the_reference_is_the_block_compressed_reference(oracle, name):
    for case, tex, nm, cutoffs, decoded, base, sn in bc.reference(name):
        got, got_sn, _ = an.compute(case, tex, nm, cutoffs, 1, diagnostics=False)
        for image in ("keys", "depth", "motion", "normal", "albedo", "specular"):
            assert np.array_equal(np.asarray(got[image]).view(np.uint8), np.asarray(base[image]).view(np.uint8)), image
        assert [got[k] for k in ("submitted", "clipped", "drawn", "rejects")] == [base[k] for k in ("submitted", "clipped", "drawn", "rejects")]
        assert (sn is None) == (got_sn is None) and (sn is None or np.array_equal(got_sn, sn))


@pytest.mark.parametrize("name", ["perspective", "with_alpha", "interpolated_basis"])
def test_without_anisotropy_the_reference_is_the_normal_map_reference(oracle, name):
    for case, tex, nm, cutoffs, base, sn, details in nc.reference(name):
        got, got_sn, _ = an.compute(case, tex, nm, cutoffs, 0, diagnostics=False)
        assert np.array_equal(got["albedo"], base["albedo"]) and np.array_equal(got["keys"], base["keys"]) and np.array_equal(got_sn, sn)


@pytest.mark.parametrize("name", list(an.CASES))
def test_case_is_what_it_is_for(oracle, name):
    an.check_case_is_what_it_is_for(name)


def test_entry_point_is_exported_and_documented():
    from plainrenderer_amd import backend
    lib = backend._load()
    assert getattr(lib, "plrf_set_scene_anisotropy") is not None
    header = open(os.path.join(ROOT, "include", "plr_frame.h")).read()
    assert "int plrf_set_scene_anisotropy(void* pipeline, uint32_t max_anisotropy);" in header and "#define PLRF_ANISOTROPY_REFERENCE 8u" in header
    from plainrenderer_amd import frame
    assert frame.ANISOTROPY_REFERENCE == 8 and hasattr(frame.FramePipeline, "set_scene_anisotropy")
