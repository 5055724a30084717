"""Block-compressed textures in the frame pipeline (plrf_set_scene_textures_formatted): 96 x 64, the scene of the normal map frame test - three meshes, a moving
camera, TAA jitter - with a BC3 albedo under an alpha cutoff, a BC1, an RGBA8 texture and two BC5 normal maps in one store.

Over three frames the compressed store must give byte-identical depth, motion, normal, albedo, specular, shadingNormal and final colour to the same pipeline fed the
numpy-decoded RGBA8 textures through plrf_set_scene_textures. An all-RGBA8 call of the new entry point equals the old entry point byte for byte. The textures are
removed by texture_count 0, dropped by plrf_set_scene_meshes, kept across a resize; a DXT5 DDS file written here with struct.pack goes from loadDDSFile into the
call; every refusal names its cause and leaves the next frame unchanged; a band pipeline refuses.
"""
import struct

import numpy as np
import pytest

import prepass_bc_cases as bc
import prepass_bc_reference as bref
import prepass_raster_cases as pc
import prepass_texture_cases as tc
import prepass_texture_reference as tref
import test_prepass_normal_frame as tnf
import test_prepass_texture_frame as ttf
from plainrenderer_amd.scene import Camera

W, H, FRAMES = ttf.W, ttf.H, 3
INVALID_ARGUMENT, UNSUPPORTED = ttf.INVALID_ARGUMENT, ttf.UNSUPPORTED
G_BUFFER = ("depth", "motion", "normal", "albedo", "specular", "shadingNormal")
CODE_OF = {bref.RGBA8: 2, bref.BC1: 13, bref.BC3: 14, bref.BC5: 15}  # PLR_FORMAT_*
CUTOFFS = [128, 0, 128]

_inputs = {}


def _scene_inputs():
    """the normal map frame test's inputs with the five textures of its store in formats: 0 a 16 x 16 BC3 whose alpha is 0 or 255 (albedo of draw 0, specular of
    draw 2 - under the cutoff it makes holes), 1 an 8 x 4 BC1 with two levels, 2 the 5 x 3 RGBA8 texture, 3 and 4 BC5 normal maps. Generated once; never modified"""
    if not _inputs:
        i = dict(tnf._scene_inputs())
        stored = [bc.full(bref.BC3, 16, 16, 91, alpha_binary=True), (bc.blocks(bref.BC1, 8, 4, 2, 92), 8, 4, 2, bref.BC1), (*i["chains"][2], bref.RGBA8),
                  bc.full(bref.BC5, 16, 16, 93), bc.full(bref.BC5, 8, 8, 94)]
        decoded = [(t[0], *t[1:4]) if t[4] == bref.RGBA8 else (bref.decode_chain(t[4], t[1], t[2], t[3], t[0]), *t[1:4]) for t in stored]
        i.update(stored=stored, decoded=decoded)
        _inputs.update(i)
    return _inputs


def _formatted(stored):
    return [(data, width, height, mips, CODE_OF[fmt]) for data, width, height, mips, fmt in stored]


def _set_scene(fp, compressed, cutoffs=CUTOFFS, normal_maps=True):
    i = _scene_inputs()
    fp.set_scene_meshes(i["meshes"], ttf._draws(i["models"]))
    if compressed:
        fp.set_scene_textures_formatted(_formatted(i["stored"]), i["uvs"], i["materials"])
    else:
        fp.set_scene_textures(i["decoded"], i["uvs"], i["materials"])
    if cutoffs is not None:
        fp.set_scene_alpha_cutoffs(cutoffs)
    if normal_maps:
        tnf._set_normal_maps(fp)


def _images(be, fp, target, width=W, height=H, shading_normal=True):
    out = tnf._g_buffer(be, fp, target, width, height, shading_normal=shading_normal)
    out.update({n: be.downloadImage(fp.image(n), 0, np.uint8).copy() for n in tnf.OUTPUTS})
    return out


def _assert_same(label, got, want):
    for name in want:
        differing = int((got[name] != want[name]).sum())
        assert differing == 0, "%s: %s differs in %d elements" % (label, name, differing)


def _expected_materials(be, fp, width=W, height=H):
    """albedo and specular of the frame the pipeline just rendered, without the alpha test, from ITS matrices, jitters and mipBias and the decoded textures"""
    i = _scene_inputs()
    case, r, _ = ttf._expected(be, fp, textured=False, width=width, height=height)
    g = np.frombuffer(fp.submitted_globals(), np.float32)
    tex = tc.textured(case, np.concatenate(i["uvs"]), i["materials"], list(i["decoded"]), mip_bias=float(g[79]))[1]
    return r, tref.sample(case, tex, r["keys"])


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_compressed_frames_equal_the_frames_of_the_decoded_textures(backend, fast):
    i = _scene_inputs()
    assert set(np.unique(i["decoded"][0][0] >> np.uint32(24)).tolist()) == {0, 255}, "texture 0 has holes"
    backend.setMathMode(fast)
    fp = None
    try:
        recorded = []
        for compressed in (False, True):
            fp = ttf._pipeline(backend, indirect_lighting_tech=1)
            _set_scene(fp, compressed)
            for k in range(FRAMES):
                tnf._run(fp, k)
                general = backend.getGeneralKernelExecutions()
                got = _images(backend, fp, (k + 1) % 2)
                if fast:
                    assert general[0] == 0, "the fast-set frame ran general kernels: %r" % (general,)
                if not compressed:
                    recorded.append((got, fp.prepass_raster_stats()))
                    continue
                assert np.frombuffer(fp.submitted_globals(), np.float32)[64:68].any(), "the TAA jitter is on"
                _assert_same("%s frame %d" % ("fast" if fast else "exact", k), got, recorded[k][0])
                assert fp.prepass_raster_stats() == recorded[k][1]
            fp.destroy()
            fp = None
        # the textures, the holes and the normal maps show
        fp = ttf._pipeline(backend, indirect_lighting_tech=1)
        fp.set_scene_meshes(i["meshes"], ttf._draws(i["models"]))
        tnf._run(fp, 0)
        plain = tnf._g_buffer(backend, fp, 1, shading_normal=False)
        first = recorded[0][0]
        assert (first["albedo"] != plain["albedo"]).sum() > 500 and (first["depth"] != plain["depth"]).sum() > 50 and (first["shadingNormal"] != first["normal"]).sum() > 500
    finally:
        if fp is not None:
            fp.destroy()
        backend.setMathMode(False)


@pytest.mark.gpu
def test_gpu_an_all_rgba8_call_equals_the_old_entry_point(backend):
    """the module's decoded textures, texture 3 as level 0 with mip_count 0 (the host builds the chain), through both entry points"""
    i = _scene_inputs()
    textures = list(i["decoded"])
    textures[3] = (textures[3][0][:256], 16, 16, 0)
    images = []
    for formatted in (False, True):
        fp = ttf._pipeline(backend, indirect_lighting_tech=1)
        try:
            fp.set_scene_meshes(i["meshes"], ttf._draws(i["models"]))
            if formatted:
                fp.set_scene_textures_formatted([(*t, CODE_OF[bref.RGBA8]) for t in textures], i["uvs"], i["materials"])
            else:
                fp.set_scene_textures(textures, i["uvs"], i["materials"])
            fp.set_scene_alpha_cutoffs(CUTOFFS)
            tnf._set_normal_maps(fp)
            tnf._run(fp, 0)
            images.append(_images(backend, fp, 1))
        finally:
            fp.destroy()
    _assert_same("all RGBA8", images[1], images[0])
    assert (images[0]["shadingNormal"] != images[0]["normal"]).sum() > 500


@pytest.mark.gpu
def test_gpu_compressed_textures_removed_dropped_and_kept(backend):
    i = _scene_inputs()
    fp = ttf._pipeline(backend)
    try:
        _set_scene(fp, True, cutoffs=None, normal_maps=False)
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        r, s = _expected_materials(backend, fp)
        ttf._assert_materials("compressed", ttf._g_buffer(backend, fp, 1), s["albedo"], s["specular"])
        assert (s["albedo"] != r["albedo"]).sum() > 200
        # texture_count 0: the constant words again
        fp.set_scene_textures_formatted([], [], [])
        fp.frame(i["cams"][2], 1.0 / 60.0, 0.5 + 1.0 / 60.0)
        case, r, _ = ttf._expected(backend, fp, textured=False)
        ttf._assert_materials("textures removed", ttf._g_buffer(backend, fp, 0), r["albedo"], r["specular"])
        # set again; plrf_set_scene_meshes drops them, the same scene given again included
        fp.set_scene_textures_formatted(_formatted(i["stored"]), i["uvs"], i["materials"])
        fp.set_scene_meshes(i["meshes"], ttf._draws(i["models"]))
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5 + 2.0 / 60.0)
        case, r, _ = ttf._expected(backend, fp, textured=False)
        ttf._assert_materials("after plrf_set_scene_meshes", ttf._g_buffer(backend, fp, 1), r["albedo"], r["specular"])
        # the old entry point replaces a compressed store, and the new one an RGBA8 store
        fp.set_scene_textures_formatted(_formatted(i["stored"]), i["uvs"], i["materials"])
        fp.set_scene_textures(list(tnf._scene_inputs()["chains"]), i["uvs"], i["materials"])
        fp.frame(i["cams"][2], 1.0 / 60.0, 0.5 + 3.0 / 60.0)
        case, r, s = ttf._expected(backend, fp)
        ttf._assert_materials("replaced by plrf_set_scene_textures", ttf._g_buffer(backend, fp, 0), s["albedo"], s["specular"])
        # they survive a resize
        fp.set_scene_textures_formatted(_formatted(i["stored"]), i["uvs"], i["materials"])
        fp.set_resolution(70, 50)
        fp.apply_changes()
        cam = Camera.look((15.06, -6.98, -5.9), (0.004, 0.16, 1.0), aspect=70 / 50)
        fp.frame(cam, 1.0 / 60.0, 0.5 + 4.0 / 60.0)
        r, s = _expected_materials(backend, fp, 70, 50)
        ttf._assert_materials("after a resize to 70 x 50", ttf._g_buffer(backend, fp, 1, 70, 50), s["albedo"], s["specular"])
        assert (s["albedo"] != r["albedo"]).sum() > 100
    finally:
        fp.destroy()


def dxt5_dds(width, height, mips, payload):
    """a legacy DDS file: magic, the 124-byte header with the fourCC DXT5 in its pixel format, the blocks of all levels"""
    caps, height_, width_, pixelformat, mipcount = 0x1, 0x2, 0x4, 0x1000, 0x20000
    pixel_format = struct.pack("<8I", 32, 0x4, 0x35545844, 0, 0, 0, 0, 0)
    header = struct.pack("<7I", 124, caps | height_ | width_ | pixelformat | mipcount, height, width, 0, 1, mips) + b"\0" * 44 + pixel_format + struct.pack("<5I", 0x1000 | 0x8 | 0x400000, 0, 0, 0, 0)
    assert len(header) == 124
    return struct.pack("<I", 0x20534444) + header + payload


@pytest.mark.gpu
def test_gpu_a_dxt5_dds_file_goes_from_the_loader_into_the_call(backend, tmp_path):
    from plainrenderer_amd import ImageFormat, image_io
    i = _scene_inputs()
    blocks, width, height, mips, _ = i["stored"][0]
    path = tmp_path / "albedo.dds"
    path.write_bytes(dxt5_dds(width, height, mips, blocks))
    desc, payload = image_io.load_dds_file(path)
    assert (desc.format, desc.width, desc.height, desc.manualMipCount) == (ImageFormat.BC3, 16, 16, 5) and payload.tobytes() == blocks
    loaded = [(payload, desc.width, desc.height, desc.manualMipCount, desc.format)] + _formatted(i["stored"])[1:]
    fp = ttf._pipeline(backend)
    try:
        fp.set_scene_meshes(i["meshes"], ttf._draws(i["models"]))
        fp.set_scene_textures_formatted(loaded, i["uvs"], i["materials"])
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        r, s = _expected_materials(backend, fp)
        ttf._assert_materials("from a DDS file", ttf._g_buffer(backend, fp, 1), s["albedo"], s["specular"])
        # level 0 of the file through the host decoder is what the reference decoded
        level0 = image_io.decode_bc_to_rgba8(desc.format, 16, 16, payload[:image_io.bc_level_bytes(desc.format, 16, 16)])
        assert np.array_equal(level0.reshape(-1), i["decoded"][0][0][:256])
    finally:
        fp.destroy()


@pytest.mark.gpu
def test_gpu_refusals_name_their_cause_and_change_nothing(backend):
    from plainrenderer_amd.backend import PlrError
    from plainrenderer_amd.frame import FramePipeline
    i = _scene_inputs()
    fp = ttf._pipeline(backend)
    try:
        def refused(call, code, *words):
            with pytest.raises(PlrError) as e:
                call()
            assert e.value.code == code, e.value
            assert all(w in str(e.value) for w in words), e.value

        stored, uvs, materials = _formatted(i["stored"]), i["uvs"], i["materials"]
        change = lambda k, **f: [tuple(f.get(n, v) for n, v in zip(("data", "width", "height", "mips", "format"), t)) if j == k else t for j, t in enumerate(stored)]
        refused(lambda: fp.set_scene_textures_formatted(stored, uvs, materials), INVALID_ARGUMENT, "no scene set")
        fp.set_scene_meshes(i["meshes"], ttf._draws(i["models"]))
        fp.set_scene_textures_formatted(stored, uvs, materials)
        refused(lambda: fp.set_scene_textures_formatted(change(1, format=1), uvs, materials), INVALID_ARGUMENT, "unknown format", "texture 1", "format 1")
        refused(lambda: fp.set_scene_textures_formatted(change(0, mips=0), uvs, materials), INVALID_ARGUMENT, "mip_count 0 on a compressed texture", "texture 0")
        refused(lambda: fp.set_scene_textures_formatted(change(3, data=stored[3][0][:-16]), uvs, materials), INVALID_ARGUMENT, "bytes mismatch", "texture 3")
        refused(lambda: fp.set_scene_textures_formatted(change(2, data=np.zeros(16, np.uint32)), uvs, materials), INVALID_ARGUMENT, "bytes mismatch", "texture 2", "64 bytes", "hold 60")
        refused(lambda: fp.set_scene_textures_formatted(change(1, mips=5), uvs, materials), INVALID_ARGUMENT, "too many mips", "texture 1", "at most 4")
        refused(lambda: fp.set_scene_textures_formatted(change(4, width=0), uvs, materials), INVALID_ARGUMENT, "texture size", "texture 4", "0 x 8")
        refused(lambda: fp.set_scene_textures_formatted(change(4, data=b""), uvs, materials), INVALID_ARGUMENT, "null texels", "texture 4")
        refused(lambda: fp.set_scene_textures_formatted(stored, uvs[:2], materials), INVALID_ARGUMENT, "mesh count 2", "mesh count 3")
        refused(lambda: fp.set_scene_textures_formatted(stored, uvs, materials + [(0, 0)]), INVALID_ARGUMENT, "draw count 4", "draw count 3")
        refused(lambda: fp.set_scene_textures_formatted(stored, uvs, [(0, 1), (5, 2), (1, tref.NONE)]), INVALID_ARGUMENT, "material texture index", "draw 1", "texture 5 of 5")
        bad = [u.copy() for u in uvs]
        bad[2][7, 1] = np.nan
        refused(lambda: fp.set_scene_textures_formatted(stored, bad, materials), INVALID_ARGUMENT, "non-finite UV", "vertex 7 of mesh 2")
        # the textures set before the refusals are the ones the next frame samples
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        r, s = _expected_materials(backend, fp)
        ttf._assert_materials("after refused calls", ttf._g_buffer(backend, fp, 1), s["albedo"], s["specular"])
    finally:
        fp.destroy()
    band = FramePipeline(backend, W, H, band_row_begin=0, band_row_end=H, **ttf.FP_ARGS)
    try:
        with pytest.raises(PlrError) as e:
            band.set_scene_textures_formatted(_formatted(i["stored"]), i["uvs"], i["materials"])
        assert e.value.code == UNSUPPORTED and "band" in str(e.value)
    finally:
        band.destroy()
