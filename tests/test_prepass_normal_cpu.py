"""The normal map reference (tests/prepass_normal_reference.py) on its own, the input conditions of the GPU cases (tests/prepass_normal_cases.py), the host's
validation, bitangent derivation and packing under a sanitizer, the mesh generators' tangents, and the entry point at the C boundary; no GPU."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import prepass_normal_cases as nc
import prepass_normal_reference as nref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(nc.CASES))
def test_cases_are_what_they_are_for(name):
    """the input conditions of the GPU test, the share of pixels that differ from `normal` included: an implementation that copies `normal` does not pass"""
    nc.check_case_is_what_it_is_for(name)


@pytest.mark.parametrize("decode", [nref.DECODE_REFERENCE, nref.DECODE_UNIT])
@pytest.mark.parametrize("texel", nc.FLAT_TEXELS)
def test_flat_codes_by_hand(texel, decode):
    """the expected word from math.sqrt and Python floats, not from the reference module"""
    cx, cy = texel
    x, y = cx / 255.0, cy / 255.0
    if decode == nref.DECODE_REFERENCE:
        radicand = ((1.0 - x * x) + y) + y
        assert radicand >= 0.0, "the radicand is never negative for codes"
        m = [2.0 * x - 1.0, 2.0 * y - 1.0, 2.0 * math.sqrt(radicand) - 1.0]
    else:
        q = (1.0 - (2.0 * x - 1.0) * (2.0 * x - 1.0)) - (2.0 * y - 1.0) * (2.0 * y - 1.0)
        m = [2.0 * x - 1.0, 2.0 * y - 1.0, math.sqrt(q) if q > 0 else 0.0]
    length = math.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
    want = sum(nc.unorm8_half(v / length) << (8 * k) for k, v in enumerate(m)) | (255 << 24)
    runs = nc.reference("flat_codes")
    k = (0 if decode == nref.DECODE_REFERENCE else len(nc.FLAT_TEXELS)) + nc.FLAT_TEXELS.index(texel)
    case, tex, nm, cutoffs, base, sn, d = runs[k]
    assert nm["decode"] == decode and int(tex["texels"][0]) & 0xFFFF == cx | (cy << 8)
    assert (base["keys"] != 0).all() and (sn == want).all(), "%08x, by hand %08x" % (int(sn[0, 0]), want)


def test_the_radicand_of_the_reference_decode_is_never_negative_for_codes():
    c = np.arange(256, dtype=np.float64) / 255.0
    x, y = np.meshgrid(c, c)
    assert (((1.0 - x * x) + y) + y >= 0).all() and (((1.0 - x * x) + y) + y).min() == 0.0


def test_derived_bitangents_follow_the_written_rule():
    t = np.array([(1, 0, 0), (0, 0, 0), (0, 2, 0), (1, 1, 1)], np.float32)
    n = np.array([(0, 0, 1), (0, 0, 1), (0, 0, 0.5), (2, 2, 2)], np.float32)
    b = nref.derive_bitangents(t, n)
    assert b.dtype == np.float32 and b.tolist() == [[0, -1, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0]]


@pytest.mark.parametrize("generator", ["box", "uv_sphere", "torus"])
def test_mesh_generators_return_unit_tangents_along_increasing_u(generator):
    from plainrenderer_amd import meshes
    args = dict(box=((1.0, 1.5, 0.75),), uv_sphere=(1.25,), torus=(1.5, 0.5))[generator]
    kwargs = dict(box=dict(subdiv=3), uv_sphere=dict(segments=12, rings=6), torus=dict(segments=10, sides=6))[generator]
    plain = getattr(meshes, generator)(*args, **kwargs)
    plain_uv = getattr(meshes, generator)(*args, with_uvs=True, **kwargs)
    out = getattr(meshes, generator)(*args, with_uvs=True, with_tangents=True, **kwargs)
    assert len(out) == len(plain_uv) + 1 and all(np.array_equal(a, b) for a, b in zip(out, plain_uv)), "the other outputs do not change"
    assert len(getattr(meshes, generator)(*args, with_tangents=True, **kwargs)) == len(plain) + 1
    pos, idx, uvs, tangents = (np.asarray(a) for a in (out[0], out[1], out[2], out[-1]))
    pos, uvs, tangents = pos.reshape(-1, 3).astype(np.float64), uvs.reshape(-1, 2).astype(np.float64), tangents.reshape(-1, 3).astype(np.float64)
    assert tangents.shape == pos.shape and np.asarray(out[-1]).dtype == np.float32
    lengths = np.linalg.norm(tangents, axis=1)
    assert np.allclose(lengths, 1.0, atol=1e-6), "unit tangents"
    # along increasing u: over every triangle edge that changes u and not v, the tangents of its ends point the way u grows
    tri = np.asarray(idx, np.int64).reshape(-1, 3)
    checked = 0
    for a, b in ((0, 1), (1, 2), (2, 0)):
        va, vb = tri[:, a], tri[:, b]
        du, dv = uvs[vb, 0] - uvs[va, 0], uvs[vb, 1] - uvs[va, 1]
        sel = (np.abs(dv) < 1e-9) & (np.abs(du) > 1e-9) & (np.abs(du) < 0.5)  # (not the seam column, where u runs back to 0)
        edge = (pos[vb[sel]] - pos[va[sel]]) * np.sign(du[sel])[:, None]
        long_enough = np.linalg.norm(edge, axis=1) > 1e-6
        dots = ((tangents[va[sel]] + tangents[vb[sel]]) * edge).sum(axis=1)[long_enough]
        assert (dots > 0).all()
        checked += int(long_enough.sum())
    assert checked > 20


def test_the_host_validation_runs_clean_under_the_sanitizers(tmp_path):
    compiler = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert compiler, "no host C++ compiler"
    exe = str(tmp_path / "scene_normal_check")
    build = subprocess.run([compiler, "-std=c++17", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tools", "scene_normal_check.cpp"), os.path.join(ROOT, "plainrenderer_amd", "csrc", "frontend", "scene_packing.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "scene_normal_check: ok", run.stdout + run.stderr


def test_the_normal_map_entry_point_is_exported():
    from plainrenderer_amd import backend
    lib = backend._load()
    assert getattr(lib, "plrf_set_scene_normal_maps") is not None
    from plainrenderer_amd.frame import NORMAL_DECODE_REFERENCE, NORMAL_DECODE_UNIT, FramePipeline, PlrfSceneMaterial
    assert (NORMAL_DECODE_REFERENCE, NORMAL_DECODE_UNIT) == (1, 2) and hasattr(FramePipeline, "set_scene_normal_maps")
    assert C.sizeof(PlrfSceneMaterial) == 8, "materials keeps its 8-byte stride"
    with open(os.path.join(ROOT, "include", "plr_frame.h")) as fh:
        header = fh.read()
    assert "#define PLRF_NORMAL_DECODE_REFERENCE 1u" in header and "#define PLRF_NORMAL_DECODE_UNIT 2u" in header
    assert "int plrf_set_scene_normal_maps(void* pipeline, const float* const* mesh_tangents, const float* const* mesh_bitangents, uint32_t mesh_count," in header
