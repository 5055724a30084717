""""sdfInstanceUpdate.comp" and "sceneMeanAlbedo.comp" through the C-ABI against tests/scene_sdf_reference.py, in both kernel sets, byte for byte.

The instance pass: the cases of tests/scene_sdf_cases.py - 1, 63, 64, 65 and 257 instances, an instance map that is not the identity, no instance at all; nine
matrices (one whose inverse leaves fp32) on three boxes; the mean albedo from an override, from the mean albedo buffer and from the constant word. Both output
buffers are compared whole: the header, the records and the prefilled bytes beyond instance n - 1, which must be unchanged.
The mean albedo pass: the store of the cases (RGBA8 at aligned and unaligned addresses, BC1 / BC3 / BC5, a level that is no multiple of 4, a texture no draw
names, two draws that share one) with one and with three groups per texture - the sums are integers, the result may not depend on the split -, the RGBA8
textures alone under a pass record without format codes, and a 1024 x 1024 texture of (255, 255, 255, 255) whose sums must be 255 * 2^20.
The launchers refuse a missing or undersized binding with a message.
"""
import struct

import numpy as np
import pytest

import scene_sdf_cases as sc
import scene_sdf_reference as ref
from util import ComputePassExecution, RenderPassResources, StorageBufferResource

F32, U32 = np.float32, np.uint32


def _buffer(be, data, minimum=16):
    data = bytes(data)
    data += bytes(max(minimum, (len(data) + 15) // 16 * 16) - len(data))
    return be.createStorageBuffer(len(data), data)


def gpu_instance_pass(be, case, drop=None, shrink=None, dispatch=None):
    """-> (instance buffer bytes, world box bytes). drop: a binding that is left out; shrink: (binding, bytes) a buffer created too small"""
    n, draws = len(case["table"]), case["models"].shape[0]
    textures = case["means"].shape[0]
    sizes = {0: case["matrices"].astype(F32).tobytes(), 1: sc.table_bytes(case["table"]), 2: case["draw_records"].astype(U32).tobytes(), 3: case["overrides"].astype(F32).tobytes(),
             4: case["instances_prefill"], 5: case["bbs_prefill"], 6: case["materials"].astype(U32).tobytes(), 7: case["means"].astype(F32).tobytes()}
    if shrink:
        sizes[shrink[0]] = sizes[shrink[0]][:shrink[1]]
    handles = {}
    for binding, data in sizes.items():
        if binding == drop:
            continue
        exact = shrink is not None and binding == shrink[0]
        handles[binding] = be.createStorageBuffer(len(data), data) if exact else _buffer(be, data)
    p = be.createComputePass("sdfInstanceUpdate.comp", [], "SDF instance update")
    be.newFrame()
    exe = ComputePassExecution(p, RenderPassResources(storageBuffers=[StorageBufferResource(h, b not in (4, 5), b) for b, h in handles.items()]),
                               struct.pack("<3I", n, draws, textures), dispatch or ((max(n, 1) + 63) // 64, 1, 1))
    be.setComputePassExecution(exe)
    be.prepareForDrawcallRecording()
    be.renderFrame()
    return (be.downloadStorageBuffer(handles[4], len(case["instances_prefill"])).tobytes(), be.downloadStorageBuffer(handles[5], len(case["bbs_prefill"])).tobytes())


def _first_difference(got, want, stride, header):
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    at = int(np.argmax(a != b))
    return "byte %d (instance %d, byte %d of its record)" % (at, (at - header) // stride, (at - header) % stride) if at >= header else "byte %d of the header" % at


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("name", sc.INSTANCE_CASES)
def test_gpu_instances_equal_the_reference_byte_for_byte(backend, name, fast):
    case, want_inst, want_bbs = sc.instance_reference(name)
    backend.setMathMode(fast)
    try:
        inst, bbs = gpu_instance_pass(backend, case)
    finally:
        backend.setMathMode(False)
    n = len(case["table"])
    print("scene sdf instances %-9s %s: %d instances, %d + %d bytes compared" % (name, "fast" if fast else "exact", n, len(inst), len(bbs)))
    assert inst == want_inst, "sdfInstances differs from the reference at " + _first_difference(inst, want_inst, 96, 16)
    assert bbs == want_bbs, "sdfWorldBBs differs from the reference at " + _first_difference(bbs, want_bbs, 32, 0)


def gpu_mean_pass(be, table, words, formats, materials, prefill, groups, drop=None, scratch_bytes=None):
    """-> (mean albedo buffer T x 4 float32, the scratch's sums T x 4 uint64)"""
    count, draws = table.shape[0], materials.shape[0]
    handles = {0: _buffer(be, table.astype(U32).tobytes()), 1: _buffer(be, words.astype(U32).tobytes()), 2: _buffer(be, materials.astype(U32).tobytes()),
               3: be.createStorageBuffer(scratch_bytes or (count * 36 + 15) // 16 * 16, None), 4: _buffer(be, prefill.astype(F32).tobytes())}
    if formats is not None:
        handles[5] = _buffer(be, formats.astype(U32).tobytes())
    if drop is not None:
        handles.pop(drop)
    p = be.createComputePass("sceneMeanAlbedo.comp", [], "Scene mean albedo")
    be.newFrame()
    exe = ComputePassExecution(p, RenderPassResources(storageBuffers=[StorageBufferResource(h, b not in (3, 4), b) for b, h in handles.items()]),
                               struct.pack("<3I", count, draws, 0 if formats is None else 1), (groups, count, 1))
    be.setComputePassExecution(exe)
    be.prepareForDrawcallRecording()
    be.renderFrame()
    return (be.downloadStorageBuffer(handles[4], count * 16, dtype=F32).reshape(count, 4).copy(), be.downloadStorageBuffer(handles[3], count * 32, dtype=np.uint64).reshape(count, 4).copy())


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("how", ["store, 1 group", "store, 3 groups", "rgba8 alone"])
def test_gpu_mean_albedos_equal_the_reference_byte_for_byte(backend, how, fast):
    case = sc.mean_case(compressed=how != "rgba8 alone")
    backend.setMathMode(fast)
    try:
        means, sums = gpu_mean_pass(backend, case["table"], case["words"], case["formats"], case["materials"], case["prefill"], 3 if "3" in how else 1)
    finally:
        backend.setMathMode(False)
    differing = [t for t in range(means.shape[0]) if means[t].tobytes() != case["expected"][t].tobytes()]
    print("scene mean albedo %-16s %s: %d textures, entries that differ %r" % (how, "fast" if fast else "exact", means.shape[0], differing))
    assert not differing, "texture %d: %r, the reference has %r" % (differing[0], means[differing[0]], case["expected"][differing[0]])
    assert (means[sc.UNUSED] == sc.SENTINEL).all() and not sums[sc.UNUSED].any(), "the texture no draw names is not reduced"
    for t in (1, 5):  # the sums themselves, for the texture two draws share and for the large one
        fmt = 0 if case["formats"] is None else int(case["formats"][t])
        assert [int(v) for v in sums[t, :3]] == ref.mean_albedo_sums(ref.level0_words(case["table"][t], fmt, case["words"]))


@pytest.mark.gpu
def test_gpu_a_white_1024_texture_sums_to_255_times_2_to_the_20(backend):
    """a 32-bit per-block partial would be the thing to overflow if it were mis-sized: one group per texture takes all 2^20 texels"""
    table = np.array([[0, 1024, 1024, 1]], U32)
    words = np.full(1024 * 1024, 0xFFFFFFFF, U32)
    materials = np.array([[0, sc.NONE]], U32)
    for groups in (1, 16):
        means, sums = gpu_mean_pass(backend, table, words, None, materials, np.full((1, 4), sc.SENTINEL, F32), groups)
        assert [int(v) for v in sums[0]] == [255 << 20, 255 << 20, 255 << 20, 0], (groups, sums)
        assert means[0].tobytes() == np.array([1, 1, 1, 0], F32).tobytes()


@pytest.mark.gpu
def test_gpu_launchers_refuse_what_they_cannot_run(backend):
    from plainrenderer_amd.backend import PlrError
    case = sc.instance_reference("65")[0]
    with pytest.raises(PlrError, match="instance table"):
        gpu_instance_pass(backend, case, drop=1)
    with pytest.raises(PlrError, match="sdfInstances"):
        gpu_instance_pass(backend, case, shrink=(4, 16 + 96 * 64))
    with pytest.raises(PlrError, match="sdfWorldBBs"):
        gpu_instance_pass(backend, case, shrink=(5, 32 * 64))
    with pytest.raises(PlrError, match="mainPassMatrices"):
        gpu_instance_pass(backend, case, shrink=(0, 192 * 64))
    with pytest.raises(PlrError, match="mean albedos"):
        gpu_instance_pass(backend, case, drop=7)
    with pytest.raises(PlrError, match="a lane per instance"):
        gpu_instance_pass(backend, case, dispatch=(1, 1, 1))
    mean = sc.mean_case()
    args = (mean["table"], mean["words"], mean["formats"], mean["materials"], mean["prefill"], 1)
    with pytest.raises(PlrError, match="texture formats"):
        gpu_mean_pass(backend, *args, drop=5)
    with pytest.raises(PlrError, match="scratch"):
        gpu_mean_pass(backend, *args, scratch_bytes=13 * 32)
    with pytest.raises(PlrError, match="texels"):
        gpu_mean_pass(backend, *args, drop=1)
