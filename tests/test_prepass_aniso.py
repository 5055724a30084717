"""Anisotropic filtering of the "depthPrepassRaster.comp" pass through the C-ABI against tests/prepass_aniso_reference.py, in both math modes: all six images
(shadingNormal where the case has a normal map) and the four counters must be bit-identical to the reference, and no pixel is left out. The cases and what each
is for: tests/prepass_aniso_cases.py.

A record with a push of 24 bytes or fewer, or with maxAnisotropy 0 or 1, is the pass it was; 2 .. 16 selects the anisotropic kernels, which need textureCount > 0
and take an all-RGBA8 store (textureFormats 0, nothing bound at 14) as well as a mixed one; a value above 16 is refused by name.
"""
import struct

import numpy as np
import pytest

import prepass_aniso_cases as an
import test_prepass_bc as tpb
import test_prepass_normal as tpn
import test_prepass_raster as tpr


def push_of(case, tex, nm, cutoffs, A, words=7):
    draws, triangles = tpn.counts_of(case)
    return struct.pack("<7I", draws, triangles, tex["texture_count"], 0 if cutoffs is None else 1, 0 if nm is None else nm["decode"], 1 if "formats" in tex else 0, A)[:4 * words]


def gpu_aniso(be, run, A=None, words=7, **how):
    case, tex, nm, cutoffs = run[:4]
    return tpb.gpu_bc(be, case, tex, nm, cutoffs, push=push_of(case, tex, nm, cutoffs, run[4] if A is None else A, words), **how)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("name", list(an.CASES))
def test_gpu_anisotropic_prepass_is_bit_identical_to_the_reference(backend, name, fast):
    an.check_case_is_what_it_is_for(name)
    backend.setMathMode(fast)
    try:
        for k, run in enumerate(an.reference(name)):
            label = "aniso %s[%d] %s" % (name, k, "fast" if fast else "exact")
            out, counted = gpu_aniso(backend, run)
            general = backend.getGeneralKernelExecutions()
            tpb.compare_six(label, out, counted, run[5], run[6])
            if fast:
                assert general[0] == 0, "the fast set ran a general kernel: %r" % (general,)
            if name == "face_on":  # N = 1 everywhere: the bytes of the same case pushed without the seventh word
                plain, plain_counted = gpu_aniso(backend, run, words=6)
                for image in tpr.IMAGES:
                    assert out[image].tobytes() == plain[image].tobytes(), "%s: %s differs from the isotropic pass'" % (label, image)
                assert counted == plain_counted
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_a_record_with_max_anisotropy_0_or_1_is_the_pass_it_was(backend, fast):
    """the 28-byte push with the seventh word at 0 and at 1 gives the bytes of the 24-byte push: an all-RGBA8 store, an alpha-tested BC3 one, a normal-mapped one"""
    backend.setMathMode(fast)
    try:
        for name in ("floor", "bc_alpha", "bc5_normal"):
            run = an.reference(name)[0]
            want, want_counted = gpu_aniso(backend, run, words=6)
            base, sn = an.isotropic(run)
            tpb.compare_six("%s, 24-byte push" % name, want, want_counted, base, sn)
            for A in (0, 1):
                out, counted = gpu_aniso(backend, run, A=A)
                for image in want:
                    assert want[image] is None or out[image].tobytes() == want[image].tobytes(), "%s, maxAnisotropy %d: %s" % (name, A, image)
                assert counted == want_counted
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_all_rgba8_store_without_binding_14(backend, fast):
    """textureFormats 0 with maxAnisotropy 8: the anisotropic kernels run with no format buffer - plain, alpha-tested and normal-mapped"""
    import prepass_alpha_cases as ac
    import prepass_normal_cases as nc
    import prepass_normal_reference as nref
    backend.setMathMode(fast)
    try:
        case, uvs = an.floor_case(64, 48)
        case = nc.with_normals(case, (0.0, -1.0, 0.0))
        _, tex = an.tc.textured(case, uvs, [(0, 1)], [an.random_chain(64, 21), an.random_chain(32, 22)])
        nm = nc.normal_inputs(case, (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), [1], nref.DECODE_UNIT)
        for label, normal_inputs, cutoffs in (("plain", None, None), ("alpha", None, np.array([ac.REFERENCE_CUTOFF], np.uint32)), ("normal", nm, None),
                                              ("alpha and normal", nm, np.array([ac.REFERENCE_CUTOFF], np.uint32))):
            run = (case, tex, normal_inputs, cutoffs, 8)
            base, sn, _ = an.compute(*run, diagnostics=False)
            assert "formats" not in tex and push_of(*run)[20:] == struct.pack("<2I", 0, 8)
            out, counted = gpu_aniso(backend, run, omit=(tpb.TEXTURE_FORMATS,))
            tpb.compare_six("aniso rgba8 %s %s" % (label, "fast" if fast else "exact"), out, counted, base, sn)
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
def test_gpu_launcher_refuses_by_name_and_leaves_nothing_behind(backend):
    from plainrenderer_amd.backend import PlrError
    run = an.reference("floor")[0]
    case, tex = run[:2]
    with pytest.raises(PlrError, match=r"depthPrepassRaster: maxAnisotropy is 17, it must be 0 or 1 \(isotropic trilinear filtering\) or 2 \.\. 16"):
        gpu_aniso(backend, run, A=17)
    with pytest.raises(PlrError, match=r"depthPrepassRaster: maxAnisotropy is 4294967295"):
        gpu_aniso(backend, run, A=0xFFFFFFFF)
    with pytest.raises(PlrError, match=r"depthPrepassRaster: maxAnisotropy is set and textureCount is 0"):
        tpb.gpu_bc(backend, case, tex, push=struct.pack("<7I", *tpn.counts_of(case), 0, 0, 0, 0, 8))
    with pytest.raises(PlrError, match=r"depthPrepassRaster: maxAnisotropy is set and textureCount is 0"):
        tpb.gpu_bc(backend, case, tex, push=struct.pack("<7I", *tpn.counts_of(case), 0, 0, 0, 0, 2))
    # a refusal leaves nothing behind
    out, counted = gpu_aniso(backend, run)
    tpb.compare_six("floor after the refusals", out, counted, run[5], run[6])
