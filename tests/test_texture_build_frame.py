"""The texture store built on the GPU in whole frames (plrf_build_scene_textures): 96 x 64, the scene of the block-compressed frame test - three meshes, a moving
camera, TAA jitter, an alpha cutoff on draws 0 and 2, two normal maps - with every texture given as RGBA8 level 0 and mip_count 0.

Stored as RGBA8 the frames must equal, byte for byte in every G-buffer image and every output, the frames of plrf_set_scene_textures fed the same level 0 (the
host's chain). Stored as BC3 (under the cutoff), BC1, RGBA8 and BC5 (the normal maps) they must equal the frames of plrf_set_scene_textures_formatted fed the
levels the numpy reference encodes. With a scene SDF set, the instances' mean albedos - "sceneMeanAlbedo.comp" runs behind the build passes - are equal too.
"""
import numpy as np
import pytest

import prepass_bc_reference as bref
import test_prepass_bc_frame as tbf
import test_prepass_normal_frame as tnf
import test_prepass_texture_frame as ttf
import texture_build_reference as xref

FRAMES = 2
RGBA8, BC1, BC3, BC5 = bref.RGBA8, bref.BC1, bref.BC3, bref.BC5
CODE_OF = tbf.CODE_OF
STORED = [BC3, BC1, RGBA8, BC5, BC5]


def _level0_sources(stored):
    """level 0 of the block-compressed frame test's decoded textures (texture 0's alpha is 0 or 255), each to be stored as stored[t]"""
    i = tbf._scene_inputs()
    return [(np.asarray(texels, np.uint32)[:w * h], w, h, 0, RGBA8, fmt) for (texels, w, h, _), fmt in zip(i["decoded"], stored)]


def _run(backend, set_textures, sdf=False):
    """the images of FRAMES frames and, with sdf, the SDF instances after the last"""
    from plainrenderer_amd.frame import SDF_BAKE
    i = tbf._scene_inputs()
    fp = ttf._pipeline(backend, indirect_lighting_tech=1)
    try:
        fp.set_scene_meshes(i["meshes"], ttf._draws(i["models"]))
        set_textures(fp)
        fp.set_scene_alpha_cutoffs(tbf.CUTOFFS)
        tnf._set_normal_maps(fp)
        if sdf:
            fp.set_scene_sdf([SDF_BAKE] * len(i["meshes"]))
        frames = []
        for k in range(FRAMES):
            tnf._run(fp, k)
            frames.append(tbf._images(backend, fp, (k + 1) % 2))
        instances = backend.downloadStorageBuffer(fp.storage_buffer("sdfInstances"), 16 + 96 * len(i["models"])).tobytes() if sdf else None
        return frames, instances, fp.texture_build_stats()
    finally:
        fp.destroy()


@pytest.mark.gpu
def test_gpu_an_rgba8_store_built_on_the_gpu_renders_as_the_host_s_chain(backend):
    i = tbf._scene_inputs()
    sources = _level0_sources([RGBA8] * 5)
    want, _, none = _run(backend, lambda fp: fp.set_scene_textures([s[:4] for s in sources], i["uvs"], i["materials"]))
    got, _, stats = _run(backend, lambda fp: fp.build_scene_textures([(d, w, h, m, CODE_OF[f], CODE_OF[s]) for d, w, h, m, f, s in sources], i["uvs"], i["materials"]))
    assert none["mip_chain_launches"] == 0 and stats["mip_chain_launches"] == 4 and stats["block_encode_launches"] == 0 and stats["staging_bytes"] == 0
    for k in range(FRAMES):
        tbf._assert_same("RGBA8 frame %d" % k, got[k], want[k])
    assert (want[0]["shadingNormal"] != want[0]["normal"]).sum() > 500 and np.unique(want[0]["albedo"]).size > 100


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_a_compressed_store_built_on_the_gpu_renders_as_the_reference_encoded_levels(backend, fast):
    i = tbf._scene_inputs()
    sources = _level0_sources(STORED)
    encoded = [xref.store_levels(s) for s in sources]
    assert [e[4] for e in encoded] == STORED and [e[3] for e in encoded] == [5, 4, 3, 5, 4]
    alpha = bref.decode_chain(BC3, 16, 16, 1, encoded[0][0][:256]) >> np.uint32(24)
    assert set(np.unique(alpha).tolist()) == {0, 255}, "two alpha values encode exactly: the cutoff makes holes"
    backend.setMathMode(fast)
    try:
        want, want_instances, _ = _run(backend, lambda fp: fp.set_scene_textures_formatted([(d, w, h, m, CODE_OF[f]) for d, w, h, m, f in encoded], i["uvs"], i["materials"]), sdf=True)
        got, got_instances, stats = _run(backend, lambda fp: fp.build_scene_textures([(d, w, h, m, CODE_OF[f], CODE_OF[s]) for d, w, h, m, f, s in sources], i["uvs"], i["materials"]),
                                         sdf=True)
    finally:
        backend.setMathMode(False)
    assert stats["mip_chain_launches"] == 4 and stats["block_encode_launches"] == 1
    for k in range(FRAMES):
        tbf._assert_same("compressed frame %d" % k, got[k], want[k])
    records = [np.frombuffer(b, np.uint32)[4:].reshape(-1, 24).copy() for b in (got_instances, want_instances)]
    for r in records:
        r[:, 3] = 0  # the volume's index in the global texture array: every pipeline bakes volumes of its own
    assert np.array_equal(records[0], records[1]), "the mean albedos of the built store are those of the formatted store"
    means = np.frombuffer(got_instances, np.float32)[4:].reshape(-1, 24)[:, 4:7]
    assert np.unique(means, axis=0).shape[0] >= 2 and (means > 0).any()
    assert (want[0]["depth"] != 0).any() and (want[0]["shadingNormal"] != want[0]["normal"]).sum() > 500
