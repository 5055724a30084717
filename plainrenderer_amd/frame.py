"""ctypes binding of the C++ frame pipeline (include/plr_frame.h) and the upload of one synthetic scene into it.

The pipeline (plainrenderer_amd/csrc/frontend/frame_pipeline.cpp) is the host-side mirror of the reference's
RenderFrontend::prepareRenderpasses + technique classes; this module only drives it for tests and benchmarks.
"""
import ctypes as C
import struct

import numpy as np

from . import synth
from .backend import ImageHandle, PlrError, RenderBackend, _ImageHandle
from .scene import Camera


class PlrfSettings(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "shadow_map_res", "brdf_lut_res", "max_sdf_instances", "froxel_depth", "taa_enabled",
                                          "taa_use_clipping", "taa_use_motion_vector_dilation", "taa_history_sampling_tech", "taa_filter_use_tonemapping",
                                          "bloom_enabled")] + \
               [("bloom_strength", C.c_float), ("bloom_radius", C.c_float), ("sdf_half_res_trace", C.c_uint32), ("sdf_strict_influence_radius_cutoff", C.c_uint32),
                ("sdf_trace_influence_radius", C.c_float)] + \
               [(n, C.c_uint32) for n in ("diffuse_brdf", "direct_multiscatter", "indirect_lighting_tech", "use_geometry_aa", "sun_shadow_cascade_count",
                                          "run_exposure", "run_hiz", "run_gi", "run_shading", "run_taa", "run_bloom", "run_tonemap",
                                          "band_row_begin", "band_row_end", "band_gi_halo", "band_gi_history_halo", "band_color_halo", "band_post_halo",
                                          "run_light_matrix")] + [("volumetrics_max_distance", C.c_float), ("taa_use_separate_supersampling", C.c_uint32), ("taa_supersample_use_tonemapping", C.c_uint32),
                                                                              ("sdf_debug_mode", C.c_uint32), ("sdf_debug_tile_usage_with_hiz", C.c_uint32),
                                                                              ("sdf_debug_use_influence_radius", C.c_uint32), ("band_taa_history_halo", C.c_uint32), ("run_volumetrics", C.c_uint32),
                                                                              ("run_sky_luts", C.c_uint32), ("band_overlap_exchange", C.c_uint32), ("band_col_begin", C.c_uint32),
                                                                              ("band_col_end", C.c_uint32), ("band_raster", C.c_uint32), ("run_sky", C.c_uint32)]


class PlrfExchangeItem(C.Structure):
    _fields_ = [("image", _ImageHandle), ("device_ptr", C.c_void_p), ("row_begin", C.c_uint32), ("row_end", C.c_uint32), ("halo_rows", C.c_uint32),
                ("row_bytes", C.c_uint32), ("image_rows", C.c_uint32), ("col_begin", C.c_uint32), ("col_end", C.c_uint32), ("image_cols", C.c_uint32),
                ("texel_bytes", C.c_uint32)]


EXCHANGE_CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p)
EXCHANGE_HISTOGRAM, EXCHANGE_GI_TRACE, EXCHANGE_GI_TEMPORAL, EXCHANGE_GI_HISTORY, EXCHANGE_POST, EXCHANGE_DEPTH_APEX = range(6)
EXCHANGE_BEGIN, EXCHANGE_END, EXCHANGE_ID_MASK = 0x100, 0x200, 0xff  # phase bits (band_overlap_exchange)


class PlrfCamera(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("forward", C.c_float * 3), ("up", C.c_float * 3), ("right", C.c_float * 3)]


class PlrMeshData(C.Structure):  # plr_mesh_data, include/plr_sdf_bake.h
    _fields_ = [("positions", C.POINTER(C.c_float)), ("vertex_count", C.c_uint32), ("indices", C.POINTER(C.c_uint32)), ("index_count", C.c_uint32)]


class PlrfShadowDraw(C.Structure):
    _fields_ = [("mesh", C.c_uint32), ("model_matrix", C.c_float * 16)]


class PlrfShadowRasterStats(C.Structure):
    _fields_ = [("triangles_submitted", C.c_uint64), ("triangles_drawn", C.c_uint64), ("guard_band_rejects", C.c_uint64)]


class PlrfSceneMesh(C.Structure):
    _fields_ = [("positions", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)), ("vertex_count", C.c_uint32), ("indices", C.POINTER(C.c_uint32)),
                ("index_count", C.c_uint32)]


class PlrfSceneDraw(C.Structure):
    _fields_ = [("mesh", C.c_uint32), ("model_matrix", C.c_float * 16), ("albedo_rgba8", C.c_uint32), ("specular_rgba8", C.c_uint32)]


NO_TEXTURE = 0xFFFFFFFF  # PLRF_NO_TEXTURE
ALPHA_CUTOFF_REFERENCE = 128  # PLRF_ALPHA_CUTOFF_REFERENCE
NORMAL_DECODE_REFERENCE, NORMAL_DECODE_UNIT = 1, 2  # PLRF_NORMAL_DECODE_REFERENCE, PLRF_NORMAL_DECODE_UNIT
ANISOTROPY_REFERENCE = 8  # PLRF_ANISOTROPY_REFERENCE


class PlrfSceneTexture(C.Structure):
    _fields_ = [("texels", C.POINTER(C.c_uint32)), ("width", C.c_uint32), ("height", C.c_uint32), ("mip_count", C.c_uint32)]


class PlrfSceneTextureData(C.Structure):
    _fields_ = [("data", C.c_void_p), ("bytes", C.c_uint64), ("width", C.c_uint32), ("height", C.c_uint32), ("mip_count", C.c_uint32), ("format", C.c_uint32)]


class PlrfSceneTextureSource(C.Structure):
    _fields_ = [("data", C.c_void_p), ("bytes", C.c_uint64), ("width", C.c_uint32), ("height", C.c_uint32), ("mip_count", C.c_uint32), ("format", C.c_uint32),
                ("store_format", C.c_uint32)]


class PlrfTextureBuildStats(C.Structure):
    _fields_ = [("mip_chain_launches", C.c_uint32), ("block_encode_launches", C.c_uint32), ("chain_texels", C.c_uint64), ("blocks_encoded", C.c_uint64),
                ("staging_bytes", C.c_uint64)]


class PlrfSceneMaterial(C.Structure):
    _fields_ = [("albedo_texture", C.c_uint32), ("specular_texture", C.c_uint32)]


class PlrfShadowCutout(C.Structure):
    _fields_ = [("albedo_texture", C.c_uint32), ("alpha_cutoff", C.c_uint32)]


class PlrfPrepassRasterStats(C.Structure):
    _fields_ = [("triangles_submitted", C.c_uint64), ("triangles_clipped", C.c_uint64), ("subtriangles_drawn", C.c_uint64), ("rejects", C.c_uint64)]


class PlrfDrawCullingStats(C.Structure):
    _fields_ = [("draws", C.c_uint32), ("visible_draws", C.c_uint32), ("triangles", C.c_uint64), ("visible_triangles", C.c_uint64), ("culled_by_plane", C.c_uint32 * 5)]


CULL_SCENE, CULL_SHADOW_CASTERS = 1, 2  # PLRF_CULL_SCENE, PLRF_CULL_SHADOW_CASTERS


class PlrfDebugGeometryStats(C.Structure):
    _fields_ = [("submitted", C.c_uint32), ("clipped", C.c_uint32), ("rejected", C.c_uint32), ("drawn", C.c_uint32), ("fragments", C.c_uint32),
                ("pixels_written", C.c_uint32), ("pad", C.c_uint32 * 2)]


DEBUG_DRAW_BOXES, DEBUG_SDF_BOXES, DEBUG_LINES = 1, 2, 4  # PLRF_DEBUG_DRAW_BOXES, PLRF_DEBUG_SDF_BOXES, PLRF_DEBUG_LINES

SDF_BAKE = 0xFFFFFFFE  # PLRF_SDF_BAKE

NOISE_BLUE, NOISE_PERLIN = 1, 2  # PLRF_NOISE_BLUE, PLRF_NOISE_PERLIN


class PlrfSceneSdfMesh(C.Structure):
    _fields_ = [("sdf_texture", C.c_uint32)]


class PlrfSceneSdfStats(C.Structure):
    _fields_ = [("instances", C.c_uint32), ("volumes_baked", C.c_uint32), ("volume_bytes", C.c_uint64)]


class LocalExchangeGroup:
    """shared state of the in-process transport of the native exchange (include/plr_frame.h plrf_local_group_*): one per partition, created before its ranks'
    pipelines attach (FramePipeline.attach_local_rects), destroyed after they are gone"""

    def __init__(self, world):
        from .backend import _load
        self.lib = _load()
        self.handle = C.c_void_p()
        self.lib.plrf_local_group_destroy.argtypes = [C.c_void_p]
        self.lib.plrf_local_group_abort.argtypes = [C.c_void_p]
        self.lib.plrf_local_group_freeze.argtypes = [C.c_void_p, C.c_int]
        if self.lib.plrf_local_group_create(C.c_int(world), C.byref(self.handle)) != 0:
            raise PlrError("plrf_local_group_create failed")

    def abort(self):
        """wake ranks that wait for a peer which has failed"""
        if self.handle:
            self.lib.plrf_local_group_abort(self.handle)

    def freeze(self, frozen=True):
        """frozen: a rank copies from what its peers posted last instead of waiting for them (one partition timed alone with real neighbour data)"""
        self.lib.plrf_local_group_freeze(self.handle, C.c_int(int(bool(frozen))))

    def destroy(self):
        if self.handle:
            self.lib.plrf_local_group_destroy(self.handle)
            self.handle = None


class FramePipeline:
    def __init__(self, be: RenderBackend, width, height, **overrides):
        self.be, self.lib = be, be.lib
        self.lib.plrf_last_error.restype = C.c_char_p
        s = PlrfSettings()
        self._check(self.lib.plrf_default_settings(C.byref(s), C.c_uint32(width), C.c_uint32(height)))
        for k, v in overrides.items():
            if not hasattr(s, k):
                raise KeyError(k)
            setattr(s, k, v)
        self.settings = s
        self.handle = C.c_void_p()
        self._check(self.lib.plrf_create(C.byref(s), C.byref(self.handle)))
        self.width, self.height = width, height

    def _check(self, rc):
        if rc != 0:
            msg = self.lib.plrf_last_error().decode() or self.lib.plr_last_error().decode()
            err = PlrError("plrf error %d: %s" % (rc, msg))
            err.code = rc
            raise err

    def destroy(self):
        if self.handle:
            self.detach_rccl()
            self.lib.plrf_destroy(self.handle)
            self.handle = None

    # ---- native RCCL halo exchange (include/plr_frame.h, csrc/frontend/band_exchange.cpp): no Python in the frame loop
    def rccl_unique_id(self):
        """bytes of a fresh ncclUniqueId (rank 0 calls this and hands the bytes to every rank)"""
        buf = C.create_string_buffer(128)
        if self.lib.plrf_rccl_get_unique_id(buf) != 0:
            self.lib.plrf_rccl_last_error.restype = C.c_char_p
            raise PlrError("plrf_rccl_get_unique_id: " + self.lib.plrf_rccl_last_error().decode())
        return buf.raw

    def attach_rccl(self, unique_id, rank, world, frame_height, bounds=None):
        """bounds: world + 1 row boundaries of a partition chosen by the caller (tiling.balanced_bounds), or None for the equal partition"""
        self.lib.plrf_rccl_last_error.restype = C.c_char_p
        x = C.c_void_p()
        rows = (C.c_uint32 * (world + 1))(*[int(v) for v in bounds]) if bounds is not None else None
        rc = self.lib.plrf_rccl_attach_rows(self.handle, C.create_string_buffer(bytes(unique_id), 128), C.c_int(rank), C.c_int(world), C.c_uint32(frame_height), rows, C.byref(x))
        if rc != 0:
            raise PlrError("plrf_rccl_attach failed (%d): %s" % (rc, self.lib.plrf_rccl_last_error().decode()))
        self._rccl = x

    def attach_rccl_rects(self, unique_id, rank, world, frame_width, frame_height, rects):
        """the native exchange for a partition into rectangles [(x0, y0, x1, y1)] (tile rendering; plrf_rccl_attach_rects). unique_id None: LOOPBACK - no
        communicator, the pack / unpack kernels run and a device copy stands in for the links (single-GPU replay of one partition's frame)"""
        self.lib.plrf_rccl_last_error.restype = C.c_char_p
        x = C.c_void_p()
        flat = (C.c_uint32 * (4 * world))(*[int(v) for r in rects for v in r])
        uid = C.create_string_buffer(bytes(unique_id), 128) if unique_id is not None else None
        rc = self.lib.plrf_rccl_attach_rects(self.handle, uid, C.c_int(rank), C.c_int(world), C.c_uint32(frame_width), C.c_uint32(frame_height), flat, C.byref(x))
        if rc != 0:
            raise PlrError("plrf_rccl_attach_rects failed (%d): %s" % (rc, self.lib.plrf_rccl_last_error().decode()))
        self._rccl = x

    def attach_local_rects(self, group, rank, world, frame_width, frame_height, rects):
        """the native exchange over the IN-PROCESS transport (plrf_local_attach_rects): every rank of the partition lives in this process on one GPU (a thread each);
        group: a LocalExchangeGroup shared by the ranks"""
        self.lib.plrf_rccl_last_error.restype = C.c_char_p
        x = C.c_void_p()
        flat = (C.c_uint32 * (4 * world))(*[int(v) for r in rects for v in r])
        rc = self.lib.plrf_local_attach_rects(self.handle, group.handle, C.c_int(rank), C.c_int(world), C.c_uint32(frame_width), C.c_uint32(frame_height), flat, C.byref(x))
        if rc != 0:
            raise PlrError("plrf_local_attach_rects failed (%d): %s" % (rc, self.lib.plrf_rccl_last_error().decode()))
        self._rccl = x

    def rccl_info(self):
        """dict: rccl_ranks, rccl_version, overlap_mode, packed_regions, stream_wait_value_supported, watchdog_ms (plrf_rccl_info)"""
        names = ("rccl_ranks", "rccl_version", "overlap_mode", "packed_regions", "stream_wait_value_supported", "watchdog_ms")
        info = (C.c_int32 * len(names))()
        self._check(self.lib.plrf_rccl_get_info(self._rccl, info))
        return dict(zip(names, [int(v) for v in info]))

    def rccl_self_test_rect(self, device_ptr, pitch_bytes, texel_bytes, rect, dst_xy):
        stream = C.c_void_p()
        self.be._check(self.lib.plr_get_stream(C.byref(stream)))
        x0, y0, x1, y1 = rect
        rc = self.lib.plrf_rccl_self_test_rect(self._rccl, C.c_void_p(device_ptr), C.c_uint32(pitch_bytes), C.c_uint32(texel_bytes), C.c_uint32(x0), C.c_uint32(y0), C.c_uint32(x1),
                                               C.c_uint32(y1), C.c_uint32(dst_xy[0]), C.c_uint32(dst_xy[1]), stream)
        if rc != 0:
            self.lib.plrf_rccl_last_error.restype = C.c_char_p
            raise PlrError("plrf_rccl_self_test_rect failed (%d): %s" % (rc, self.lib.plrf_rccl_last_error().decode()))

    def detach_rccl(self):
        if getattr(self, "_rccl", None):
            self.lib.plrf_rccl_detach(self.handle, self._rccl)
            self._rccl = None

    def rccl_stats(self):
        """(bytes sent, bytes received, point-to-point exchange groups) of the last frame on this rank"""
        a, b, n = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.plrf_rccl_get_stats(self._rccl, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def rccl_self_test(self, device_ptr, row_bytes, src_row, dst_row, rows):
        stream = C.c_void_p()
        self.be._check(self.lib.plr_get_stream(C.byref(stream)))
        rc = self.lib.plrf_rccl_self_test(self._rccl, C.c_void_p(device_ptr), C.c_uint32(row_bytes), C.c_uint32(src_row), C.c_uint32(dst_row), C.c_uint32(rows), stream)
        if rc != 0:
            raise PlrError("plrf_rccl_self_test failed (%d): %s" % (rc, self.lib.plrf_rccl_last_error().decode()))

    def image(self, name):
        h = _ImageHandle()
        self._check(self.lib.plrf_get_image(self.handle, name.encode(), C.byref(h)))
        return ImageHandle(h.type, h.index)

    def storage_buffer(self, name):
        h = C.c_uint32()
        self._check(self.lib.plrf_get_storage_buffer(self.handle, name.encode(), C.byref(h)))
        return h.value

    def uniform_buffer(self, name):
        h = C.c_uint32()
        self._check(self.lib.plrf_get_uniform_buffer(self.handle, name.encode(), C.byref(h)))
        return h.value

    def add_sdf_volume(self, res, half_data):
        a = np.ascontiguousarray(half_data)
        out = C.c_uint32()
        self._check(self.lib.plrf_add_sdf_volume(self.handle, C.c_uint32(res), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), C.byref(out)))
        return out.value

    def add_sdf_volume_dds(self, path):
        """-> (global texture array index, (width, height, depth)) of a baked SDF volume stored as DDS"""
        out = C.c_uint32()
        size = (C.c_uint32 * 3)()
        self._check(self.lib.plrf_add_sdf_volume_dds(self.handle, str(path).encode(), C.byref(out), size))
        return out.value, tuple(int(v) for v in size)

    def set_sdf_scene(self, instance_bytes, bb_bytes):
        self._check(self.lib.plrf_set_sdf_scene(self.handle, instance_bytes, C.c_size_t(len(instance_bytes)), bb_bytes, C.c_size_t(len(bb_bytes))))

    def set_sun_direction(self, d):
        self._check(self.lib.plrf_set_sun_direction(self.handle, (C.c_float * 3)(*[float(x) for x in d])))

    def set_camera_intrinsic(self, fov, near, far):
        self._check(self.lib.plrf_set_camera_intrinsic(self.handle, C.c_float(fov), C.c_float(near), C.c_float(far)))

    def set_camera_cut(self):
        self._check(self.lib.plrf_set_camera_cut(self.handle))

    # ---- live changes (include/plr_frame.h plrf_set_resolution / plrf_update_settings): recorded, applied at the start of the next frame() or by apply_changes()
    def set_resolution(self, width, height):
        """resize the frame (0 in either: minimized, frames render nothing); images that follow the screen come back zero-filled, the next frame is a camera cut"""
        self._check(self.lib.plrf_set_resolution(self.handle, C.c_uint32(width), C.c_uint32(height)))
        self.width, self.height = width, height
        self.settings.width, self.settings.height = width, height

    def update_settings(self, **overrides):
        """change the settings the reference's UI edits (taa_*, bloom_*, sdf_half_res_trace, ..., plr_frame.h), starting from the current ones; any other field
        that differs raises PlrError (PLR_ERR_UNSUPPORTED), width / height too (PLR_ERR_INVALID_ARGUMENT: use set_resolution)"""
        s = PlrfSettings()
        C.memmove(C.byref(s), C.byref(self.settings), C.sizeof(PlrfSettings))
        for k, v in overrides.items():
            if not hasattr(s, k):
                raise KeyError(k)
            setattr(s, k, v)
        self._check(self.lib.plrf_update_settings(self.handle, C.byref(s)))
        self.settings = s

    def apply_changes(self):
        """apply a recorded resize / settings change now, so that inputs of the new size can be uploaded before the next frame()"""
        self._check(self.lib.plrf_apply_changes(self.handle))

    # ---- mesh shadow casters (include/plr_frame.h plrf_set_shadow_casters): the sun shadow cascades rasterised every frame by "sunShadowRaster.comp"
    def set_shadow_casters(self, meshes, draws):
        """meshes: [(positions n x 3 float32, indices uint32 triangle list)], draws: [(mesh index, 16 floats, glm column-major)]; copied. No draws: the casters
        are removed and the uploaded shadow maps are used again"""
        pos = [np.ascontiguousarray(p, np.float32).reshape(-1, 3) for p, _ in meshes]
        idx = [np.ascontiguousarray(i, np.uint32).reshape(-1) for _, i in meshes]
        m = (PlrMeshData * max(len(meshes), 1))()
        for k in range(len(meshes)):
            m[k] = PlrMeshData(pos[k].ctypes.data_as(C.POINTER(C.c_float)), pos[k].shape[0], idx[k].ctypes.data_as(C.POINTER(C.c_uint32)), idx[k].size)
        d = (PlrfShadowDraw * max(len(draws), 1))()
        for k, (mesh, matrix) in enumerate(draws):
            d[k].mesh = int(mesh)
            d[k].model_matrix = (C.c_float * 16)(*[float(v) for v in np.asarray(matrix, np.float32).reshape(16)])
        self._check(self.lib.plrf_set_shadow_casters(self.handle, m, C.c_uint32(len(meshes)), d, C.c_uint32(len(draws))))

    def set_shadow_caster_transforms(self, matrices):
        """one 16-float model matrix per draw, from the next frame on"""
        a = np.ascontiguousarray(matrices, np.float32).reshape(-1, 16)
        self._check(self.lib.plrf_set_shadow_caster_transforms(self.handle, a.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(a.shape[0])))

    def set_shadow_caster_cutouts(self, textures, mesh_uvs, cutouts):
        """alpha-tested cutouts for the casters now set. textures: as for set_scene_textures (the casters keep their own copy); mesh_uvs: one n x 2 float32 array
        or None per caster mesh; cutouts: one (albedo texture or NO_TEXTURE, alpha cutoff code 0 .. 255) per caster draw, 0: opaque, ALPHA_CUTOFF_REFERENCE = 128:
        the reference's alpha < 0.5 -> discard. Copied; from the next frame on. No textures: the cutouts are removed. The pass culls front faces: a single-sided
        card that faces the light is culled before it is tested"""
        t, u, keep = self._texture_arguments(textures, mesh_uvs)
        m = (PlrfShadowCutout * max(len(cutouts), 1))()
        for k, (albedo, cutoff) in enumerate(cutouts):
            m[k] = PlrfShadowCutout(int(albedo), int(cutoff))
        self._check(self.lib.plrf_set_shadow_caster_cutouts(self.handle, t, C.c_uint32(len(textures)), u, C.c_uint32(len(mesh_uvs)), m, C.c_uint32(len(cutouts))))

    def shadow_raster_record(self):
        """(push constant bytes, storage buffers bound) of the cascades' pass record as the last frame with casters made it: (8, 6) opaque, (12, 10) cutouts
        whose store is all RGBA8, (16, 11) a store with a compressed entry; (0, 0) before such a frame"""
        push, buffers = C.c_uint32(0), C.c_uint32(0)
        self._check(self.lib.plrf_get_shadow_raster_record(self.handle, C.byref(push), C.byref(buffers)))
        return int(push.value), int(buffers.value)

    def shadow_raster_stats(self, cascade):
        """(triangles submitted, triangles drawn, guard-band rejects) of the last frame's execution for the cascade; waits for the GPU"""
        s = PlrfShadowRasterStats()
        self._check(self.lib.plrf_get_shadow_raster_stats(self.handle, C.c_uint32(cascade), C.byref(s)))
        return int(s.triangles_submitted), int(s.triangles_drawn), int(s.guard_band_rejects)

    # ---- scene meshes (include/plr_frame.h plrf_set_scene_meshes): the G-buffer rasterised every frame by "depthPrepassRaster.comp"
    def set_scene_meshes(self, meshes, draws):
        """meshes: [(positions n x 3 float32, normals n x 3 float32 or None, indices uint32 triangle list)], draws: [(mesh index, 16 floats glm column-major,
        albedo RGBA8 word, specular RGBA8 word)]; copied. No draws: the scene is removed and the uploaded G-buffer is used again"""
        pos = [np.ascontiguousarray(m[0], np.float32).reshape(-1, 3) for m in meshes]
        nrm = [None if m[1] is None else np.ascontiguousarray(m[1], np.float32).reshape(-1, 3) for m in meshes]
        idx = [np.ascontiguousarray(m[2], np.uint32).reshape(-1) for m in meshes]
        m = (PlrfSceneMesh * max(len(meshes), 1))()
        for k in range(len(meshes)):
            if nrm[k] is not None and nrm[k].shape != pos[k].shape:
                raise ValueError("mesh %d has %d normals for %d vertices" % (k, nrm[k].shape[0], pos[k].shape[0]))
            m[k] = PlrfSceneMesh(pos[k].ctypes.data_as(C.POINTER(C.c_float)), None if nrm[k] is None else nrm[k].ctypes.data_as(C.POINTER(C.c_float)), pos[k].shape[0],
                                 idx[k].ctypes.data_as(C.POINTER(C.c_uint32)), idx[k].size)
        d = (PlrfSceneDraw * max(len(draws), 1))()
        for k, (mesh, matrix, albedo, specular) in enumerate(draws):
            d[k].mesh = int(mesh)
            d[k].model_matrix = (C.c_float * 16)(*[float(v) for v in np.asarray(matrix, np.float32).reshape(16)])
            d[k].albedo_rgba8, d[k].specular_rgba8 = int(albedo), int(specular)
        self._check(self.lib.plrf_set_scene_meshes(self.handle, m, C.c_uint32(len(meshes)), d, C.c_uint32(len(draws))))
        self._scene_mesh_count = len(meshes)  # (what set_scene_normal_maps passes when it is given neither tangents nor bitangents)

    def set_scene_mesh_transforms(self, matrices):
        """one 16-float model matrix per draw, from the next frame on"""
        a = np.ascontiguousarray(matrices, np.float32).reshape(-1, 16)
        self._check(self.lib.plrf_set_scene_mesh_transforms(self.handle, a.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(a.shape[0])))

    @staticmethod
    def _texture_arguments(textures, mesh_uvs):
        """the plrf_scene_texture array and the UV pointer array of set_scene_textures / set_shadow_caster_cutouts, and the arrays they point into"""
        tex = [np.ascontiguousarray(t[0], np.uint32).reshape(-1) for t in textures]
        uvs = [None if u is None else np.ascontiguousarray(u, np.float32).reshape(-1, 2) for u in mesh_uvs]
        t = (PlrfSceneTexture * max(len(textures), 1))()
        for k, (_, width, height, mips) in enumerate(textures):
            valid = 0 < width <= 16384 and 0 < height <= 16384 and mips <= max(int(width), int(height)).bit_length()  # (otherwise the call refuses and reads nothing)
            need = sum(max(1, int(width) >> l) * max(1, int(height) >> l) for l in range(max(1, int(mips)))) if valid else 0
            if tex[k].size and tex[k].size < need:  # (no texels at all: NULL, which the call refuses)
                raise ValueError("texture %d has %d texels for %d x %d with %d levels" % (k, tex[k].size, width, height, mips))
            t[k] = PlrfSceneTexture(tex[k].ctypes.data_as(C.POINTER(C.c_uint32)) if tex[k].size else None, int(width), int(height), int(mips))
        u = (C.POINTER(C.c_float) * max(len(uvs), 1))()
        for k, a in enumerate(uvs):
            u[k] = None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
        return t, u, (tex, uvs)

    def set_scene_textures(self, textures, mesh_uvs, materials):
        """textures: [(texels uint32 RGBA8 with R in the low byte, width, height, mip_count)] - mip_count levels back to back, or 0: level 0 only and the host builds
        the full chain; mesh_uvs: one n x 2 float32 array or None per mesh of the scene; materials: one (albedo texture, specular texture) per draw, NO_TEXTURE for
        the draw's constant word. Copied; from the next frame on. No textures: they are removed"""
        t, u, keep = self._texture_arguments(textures, mesh_uvs)
        m = (PlrfSceneMaterial * max(len(materials), 1))()
        for k, (albedo, specular) in enumerate(materials):
            m[k] = PlrfSceneMaterial(int(albedo), int(specular))
        self._check(self.lib.plrf_set_scene_textures(self.handle, t, C.c_uint32(len(textures)), u, C.c_uint32(len(mesh_uvs)), m, C.c_uint32(len(materials))))

    @staticmethod
    def _formatted_texture_arguments(textures, mesh_uvs):
        """the plrf_scene_texture_data array and the UV pointer array of set_scene_textures_formatted / set_shadow_caster_cutouts_formatted, and the arrays they
        point into"""
        def as_bytes(data, fmt):  # RGBA8 texels are uint32 words whatever integer type they come in; blocks are taken as the bytes they are
            if isinstance(data, (bytes, bytearray)):
                return np.frombuffer(data, np.uint8)
            return (np.ascontiguousarray(data, np.uint32) if int(fmt) == 2 else np.ascontiguousarray(data)).reshape(-1).view(np.uint8)
        data = [as_bytes(t[0], t[4]) for t in textures]
        uvs = [None if u is None else np.ascontiguousarray(u, np.float32).reshape(-1, 2) for u in mesh_uvs]
        t = (PlrfSceneTextureData * max(len(textures), 1))()
        for k, (_, width, height, mips, fmt) in enumerate(textures):
            t[k] = PlrfSceneTextureData(data[k].ctypes.data if data[k].size else None, data[k].size, int(width), int(height), int(mips), int(fmt))
        u = (C.POINTER(C.c_float) * max(len(uvs), 1))()
        for k, a in enumerate(uvs):
            u[k] = None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
        return t, u, (data, uvs)

    def set_shadow_caster_cutouts_formatted(self, textures, mesh_uvs, cutouts):
        """set_shadow_caster_cutouts for textures that carry a format (include/plr_frame.h plrf_set_shadow_caster_cutouts_formatted): textures as
        set_scene_textures_formatted takes them, [(data, width, height, mip_count, format)]; mesh_uvs and cutouts as for set_shadow_caster_cutouts. The alpha of a
        BC3 texel is its alpha block's code, of a BC1 or BC5 texel 255. The two calls replace one another's store; no textures: the cutouts are removed"""
        t, u, keep = self._formatted_texture_arguments(textures, mesh_uvs)
        m = (PlrfShadowCutout * max(len(cutouts), 1))()
        for k, (albedo, cutoff) in enumerate(cutouts):
            m[k] = PlrfShadowCutout(int(albedo), int(cutoff))
        self.lib.plrf_set_shadow_caster_cutouts_formatted.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        self._check(self.lib.plrf_set_shadow_caster_cutouts_formatted(self.handle, C.cast(t, C.c_void_p), C.c_uint32(len(textures)), C.cast(u, C.c_void_p), C.c_uint32(len(mesh_uvs)),
                                                                      C.cast(m, C.c_void_p), C.c_uint32(len(cutouts))))

    def set_scene_textures_formatted(self, textures, mesh_uvs, materials):
        """set_scene_textures for textures that carry a format: textures: [(data, width, height, mip_count, format)] with format an ImageFormat - RGBA8: data are
        uint32 texels as for set_scene_textures (mip_count 0: the host builds the chain); BC1, BC3, BC5: data are the bytes (any array, or bytes) of the blocks of
        mip_count >= 1 levels back to back, as image_io.load_dds_file returns them for a DXT1 / DXT5 / ATI2 file. The byte count handed over is the array's: the
        call refuses one that is not the exact size of the levels. mesh_uvs, materials, lifetime and removal as for set_scene_textures"""
        t, u, keep = self._formatted_texture_arguments(textures, mesh_uvs)
        m = (PlrfSceneMaterial * max(len(materials), 1))()
        for k, (albedo, specular) in enumerate(materials):
            m[k] = PlrfSceneMaterial(int(albedo), int(specular))
        self.lib.plrf_set_scene_textures_formatted.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        self._check(self.lib.plrf_set_scene_textures_formatted(self.handle, C.cast(t, C.c_void_p), C.c_uint32(len(textures)), C.cast(u, C.c_void_p), C.c_uint32(len(mesh_uvs)),
                                                               C.cast(m, C.c_void_p), C.c_uint32(len(materials))))

    def build_scene_textures(self, textures, mesh_uvs, materials):
        """set_scene_textures_formatted with the mip chains and the BC1 / BC3 / BC5 blocks made on the GPU (include/plr_frame.h plrf_build_scene_textures):
        textures: [(data, width, height, mip_count, format, store_format)] - an RGBA8 source is stored as RGBA8, BC1, BC3 or BC5, a compressed source as what it is;
        mip_count 0: data is level 0 and the GPU builds the chain. The next frame records the build passes; the store has the layout
        set_scene_textures_formatted gives the same textures with all their levels. mesh_uvs, materials, lifetime and removal as for set_scene_textures"""
        def as_bytes(data, fmt):
            if isinstance(data, (bytes, bytearray)):
                return np.frombuffer(data, np.uint8)
            return (np.ascontiguousarray(data, np.uint32) if int(fmt) == 2 else np.ascontiguousarray(data)).reshape(-1).view(np.uint8)
        data = [as_bytes(t[0], t[4]) for t in textures]
        uvs = [None if u is None else np.ascontiguousarray(u, np.float32).reshape(-1, 2) for u in mesh_uvs]
        t = (PlrfSceneTextureSource * max(len(textures), 1))()
        for k, (_, width, height, mips, fmt, store_fmt) in enumerate(textures):
            t[k] = PlrfSceneTextureSource(data[k].ctypes.data if data[k].size else None, data[k].size, int(width), int(height), int(mips), int(fmt), int(store_fmt))
        u = (C.POINTER(C.c_float) * max(len(uvs), 1))()
        for k, a in enumerate(uvs):
            u[k] = None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
        m = (PlrfSceneMaterial * max(len(materials), 1))()
        for k, (albedo, specular) in enumerate(materials):
            m[k] = PlrfSceneMaterial(int(albedo), int(specular))
        self.lib.plrf_build_scene_textures.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        self._check(self.lib.plrf_build_scene_textures(self.handle, C.cast(t, C.c_void_p), C.c_uint32(len(textures)), C.cast(u, C.c_void_p), C.c_uint32(len(mesh_uvs)),
                                                       C.cast(m, C.c_void_p), C.c_uint32(len(materials))))

    def read_scene_texture_store(self):
        """-> the uint32 words of the texel store as the kernels see it, whichever call made it; refused before a frame has run since that call. Waits for the GPU"""
        n = C.c_uint64()
        self.lib.plrf_read_scene_texture_store.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        self._check(self.lib.plrf_read_scene_texture_store(self.handle, None, C.c_uint64(0), C.byref(n)))
        out = np.empty(n.value, np.uint32)
        self._check(self.lib.plrf_read_scene_texture_store(self.handle, out.ctypes.data_as(C.c_void_p) if out.size else None, C.c_uint64(out.size), C.byref(n)))
        return out

    def texture_build_stats(self):
        """the last build a frame has recorded: dict(mip_chain_launches, block_encode_launches, chain_texels, blocks_encoded, staging_bytes); zeros before one"""
        s = PlrfTextureBuildStats()
        self.lib.plrf_get_texture_build_stats.argtypes = [C.c_void_p, C.c_void_p]
        self._check(self.lib.plrf_get_texture_build_stats(self.handle, C.byref(s)))
        return {name: int(getattr(s, name)) for name, _ in PlrfTextureBuildStats._fields_}

    def set_scene_alpha_cutoffs(self, cutoffs):
        """one alpha cutoff code 0 .. 255 per draw of the scene (0: opaque, ALPHA_CUTOFF_REFERENCE = 128: the reference's alpha < 0.5 -> discard); needs textures.
        Copied; from the next frame on. No cutoffs: they are removed"""
        a = np.ascontiguousarray(cutoffs, np.uint32).reshape(-1)
        self.lib.plrf_set_scene_alpha_cutoffs.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32]
        self._check(self.lib.plrf_set_scene_alpha_cutoffs(self.handle, a.ctypes.data_as(C.POINTER(C.c_uint32)) if a.size else None, C.c_uint32(a.size)))

    def set_scene_normal_maps(self, mesh_tangents, mesh_bitangents, normal_textures, decode=NORMAL_DECODE_REFERENCE):
        """normal maps for the scene and textures now set: mesh_tangents, mesh_bitangents: one n x 3 float32 array or None per mesh of the scene (the list itself
        may be None: every mesh without) - no tangents: all (0, 0, 0); no bitangents: the host derives normalize(cross(tangent, normal)); normal_textures: one
        texture index or NO_TEXTURE per draw; decode: NORMAL_DECODE_REFERENCE (the reference's reconstruction as written) or NORMAL_DECODE_UNIT. Copied; from the
        next frame on the prepass writes the "shadingNormal" image and the deferred shade reads it. No normal_textures: they are removed"""
        def pointers(arrays):
            if arrays is None:
                return None, 0, []
            keep = [None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in arrays]
            p = (C.POINTER(C.c_float) * max(len(keep), 1))()
            for k, a in enumerate(keep):
                p[k] = None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
            return p, len(keep), keep
        t, tn, keep_t = pointers(mesh_tangents)
        b, bn, keep_b = pointers(mesh_bitangents)
        n = np.ascontiguousarray(normal_textures, np.uint32).reshape(-1)
        self.lib.plrf_set_scene_normal_maps.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32]
        self._check(self.lib.plrf_set_scene_normal_maps(self.handle, None if t is None else C.cast(t, C.c_void_p), None if b is None else C.cast(b, C.c_void_p),
                                                        C.c_uint32(max(tn, bn) if t is not None or b is not None else getattr(self, "_scene_mesh_count", 0)), n.ctypes.data_as(C.POINTER(C.c_uint32)) if n.size else None, C.c_uint32(n.size),
                                                        C.c_uint32(int(decode))))

    def set_scene_anisotropy(self, max_anisotropy):
        """anisotropic filtering of every texture sample of the depth prepass: 0 or 1 off, 2 .. 16 on (ANISOTROPY_REFERENCE = 8: the reference's sampler), from the
        next recorded frame; needs neither a scene nor textures and survives every other scene call, set_resolution and update_settings"""
        self.lib.plrf_set_scene_anisotropy.argtypes = [C.c_void_p, C.c_uint32]
        self._check(self.lib.plrf_set_scene_anisotropy(self.handle, C.c_uint32(int(max_anisotropy))))

    def prepass_raster_stats(self):
        """(triangles submitted, triangles clipped, sub-triangles drawn, rejects) of the last frame's execution; waits for the GPU"""
        s = PlrfPrepassRasterStats()
        self._check(self.lib.plrf_get_prepass_raster_stats(self.handle, C.byref(s)))
        return int(s.triangles_submitted), int(s.triangles_clipped), int(s.subtriangles_drawn), int(s.rejects)

    # ---- frustum culling of draws (include/plr_frame.h plrf_set_draw_culling): "drawCulling.comp" in front of the two rasterisers
    def set_draw_culling(self, flags):
        """CULL_SCENE (1): the depth prepass's draws against the frame's own jittered viewProjection; CULL_SHADOW_CASTERS (2): the casters, per cascade, against
        that frame's light matrices. From the next frame on, until changed; 0 turns it off. The rasterisers' images do not change, their counters count the kept
        draws only"""
        self.lib.plrf_set_draw_culling.argtypes = [C.c_void_p, C.c_uint32]
        self._check(self.lib.plrf_set_draw_culling(self.handle, C.c_uint32(int(flags))))

    def draw_culling_stats(self, view):
        """dict(draws, visible_draws, triangles, visible_triangles, culled_by_plane [near, +x, -x, +y, -y]) of the last frame's cull execution for view 0 (the
        main pass) or 1 + c (cascade c); waits for the GPU. All zero for a view that is off, absent or not yet rendered"""
        s = PlrfDrawCullingStats()
        self.lib.plrf_get_draw_culling_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        self._check(self.lib.plrf_get_draw_culling_stats(self.handle, C.c_uint32(int(view)), C.byref(s)))
        return dict(draws=int(s.draws), visible_draws=int(s.visible_draws), triangles=int(s.triangles), visible_triangles=int(s.visible_triangles),
                    culled_by_plane=[int(v) for v in s.culled_by_plane])

    # ---- debug geometry (include/plr_frame.h plrf_set_debug_geometry): "debugGeometry.comp" behind the deferred shade
    def set_debug_geometry(self, flags):
        """DEBUG_DRAW_BOXES (1): the world box of every scene draw, red; DEBUG_SDF_BOXES (2): the padded world boxes of the scene SDF's instances, green;
        DEBUG_LINES (4): the segments of set_debug_lines. One-pixel lines, depth-tested, with depth write on, into the frame's colour and depth images from the
        next frame on, until changed; 0 turns it off"""
        self.lib.plrf_set_debug_geometry.argtypes = [C.c_void_p, C.c_uint32]
        self._check(self.lib.plrf_set_debug_geometry(self.handle, C.c_uint32(int(flags))))

    def set_debug_lines(self, lines):
        """an array of shape (n, 9): a.xyz, b.xyz in world space and a linear rgb per segment, copied. None or empty: the lines are removed"""
        a = np.ascontiguousarray(lines if lines is not None else np.zeros((0, 9)), np.float32)
        if a.size and (a.ndim != 2 or a.shape[1] != 9):
            raise ValueError("set_debug_lines: the lines are an array of shape (n, 9), got %r" % (a.shape,))
        a = a.reshape(-1, 9)
        self.lib.plrf_set_debug_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        self._check(self.lib.plrf_set_debug_lines(self.handle, a.ctypes.data_as(C.c_void_p) if a.shape[0] else None, C.c_uint32(a.shape[0])))

    def debug_geometry_stats(self):
        """dict(submitted, clipped, rejected, drawn, fragments, pixels_written) of the last frame that recorded the pass; waits for the GPU. All zero before one"""
        s = PlrfDebugGeometryStats()
        self.lib.plrf_get_debug_geometry_stats.argtypes = [C.c_void_p, C.c_void_p]
        self._check(self.lib.plrf_get_debug_geometry_stats(self.handle, C.byref(s)))
        return dict(submitted=int(s.submitted), clipped=int(s.clipped), rejected=int(s.rejected), drawn=int(s.drawn), fragments=int(s.fragments),
                    pixels_written=int(s.pixels_written))

    # ---- the scene's SDF (include/plr_frame.h plrf_set_scene_sdf): sdfInstances and sdfWorldBBs written every frame by "sdfInstanceUpdate.comp"
    def set_scene_sdf(self, sdf_textures):
        """one entry per mesh of the scene: an index add_sdf_volume / add_sdf_volume_dds returned, SDF_BAKE (baked now and registered), or NO_TEXTURE (the mesh
        has no SDF: its draws make no instance). The draws whose mesh has an SDF, in draw order, are the instances. None or empty: the scene SDF is removed"""
        values = [int(v) for v in (sdf_textures if sdf_textures is not None else [])]
        m = (PlrfSceneSdfMesh * max(len(values), 1))()
        for k, v in enumerate(values):
            m[k].sdf_texture = v
        self._check(self.lib.plrf_set_scene_sdf(self.handle, m, C.c_uint32(len(values))))

    def set_scene_sdf_mean_albedo(self, rgb_or_nan):
        """one (r, g, b) per draw instead of the derived mean albedo; a NaN red = derive. None or empty: the overrides are removed"""
        a = np.ascontiguousarray(rgb_or_nan if rgb_or_nan is not None else np.zeros((0, 3)), np.float32).reshape(-1, 3)
        self._check(self.lib.plrf_set_scene_sdf_mean_albedo(self.handle, a.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(a.shape[0])))

    def scene_sdf_stats(self):
        """(instances, volumes baked, bytes of the baked volumes) of the scene SDF now set; zeros without one"""
        s = PlrfSceneSdfStats()
        self._check(self.lib.plrf_get_scene_sdf_stats(self.handle, C.byref(s)))
        return int(s.instances), int(s.volumes_baked), int(s.volume_bytes)

    # ---- the frame's noise inputs (include/plr_frame.h plrf_generate_noise): "blueNoiseVoidAndCluster.comp" and "perlinNoise3D.comp"
    def generate_noise(self, seed, flags=NOISE_BLUE | NOISE_PERLIN):
        """the next frame() writes noise0 .. noise3 (NOISE_BLUE: void-and-cluster blue noise, texture t from streams 2 t and 2 t + 1 of the seed) and / or
        perlinNoise3D (NOISE_PERLIN: the 32^3 Perlin volume, 8 cells) on the GPU, once and in front of everything else; they stay until uploaded to or generated again"""
        self.lib.plrf_generate_noise.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        self._check(self.lib.plrf_generate_noise(self.handle, C.c_uint32(int(seed) & 0xFFFFFFFF), C.c_uint32(int(flags))))

    def noise_stats(self):
        """-> (4, 2, 4) uint32: {swaps, converged, ones, 0} per texture and channel of the last blue-noise generation a frame has run; waits for the GPU"""
        out = np.zeros((4, 2, 4), np.uint32)
        self.lib.plrf_get_noise_stats.argtypes = [C.c_void_p, C.c_void_p]
        self._check(self.lib.plrf_get_noise_stats(self.handle, out.ctypes.data_as(C.c_void_p)))
        return out

    def raster_window(self):
        """(x0, y0, x1, y1), half-open, in 64 x 64 tiles: the window the depth prepass of a partitioned pipeline with band_raster = 1 is restricted to"""
        out = (C.c_uint32 * 4)()
        self._check(self.lib.plrf_get_raster_window(self.handle, out))
        return tuple(int(v) for v in out)

    def frame(self, cam: Camera, delta_time=1.0 / 60.0, time=0.0):
        c = PlrfCamera()
        for name in ("position", "forward", "up", "right"):
            setattr(c, name, (C.c_float * 3)(*[float(x) for x in getattr(cam, name)]))
        self._check(self.lib.plrf_frame(self.handle, C.byref(c), C.c_float(delta_time), C.c_float(time)))

    # ---- band rendering (include/plr_frame.h)
    def set_exchange_callback(self, fn):
        """fn(exchange_id, hip_stream_ptr) -> None; called in pass order from inside frame() where neighbouring bands' rows are needed."""
        def tramp(_user, exchange_id, stream):
            try:
                fn(int(exchange_id), stream)
                return 0
            except Exception:  # an exception cannot cross the C frames; report and fail the frame
                import traceback
                traceback.print_exc()
                return -7
        self._exchange_cb = EXCHANGE_CALLBACK(tramp)  # keep alive
        self._check(self.lib.plrf_set_exchange_callback(self.handle, self._exchange_cb, None))

    def exchange_items(self, exchange_id):
        n = C.c_uint32(16)
        items = (PlrfExchangeItem * 16)()
        self._check(self.lib.plrf_get_exchange_items(self.handle, C.c_int(exchange_id), items, C.byref(n)))
        return [items[i] for i in range(n.value)]

    def histogram_exchange(self):
        ptr, size = C.c_void_p(), C.c_size_t()
        self._check(self.lib.plrf_get_histogram_exchange(self.handle, C.byref(ptr), C.byref(size)))
        return ptr.value, size.value

    def depth_apex_exchange(self):
        """(device pointer, 8): the band's {min, max} depth range, to be all-reduced in place (EXCHANGE_DEPTH_APEX)"""
        ptr, size = C.c_void_p(), C.c_size_t()
        self._check(self.lib.plrf_get_depth_apex_exchange(self.handle, C.byref(ptr), C.byref(size)))
        return ptr.value, size.value

    def submitted_globals(self):
        buf = C.create_string_buffer(340)
        self._check(self.lib.plrf_get_submitted_globals(self.handle, buf))
        return buf.raw

    def resolve_weights(self):
        w = np.zeros(9, np.float32)
        self._check(self.lib.plrf_get_resolve_weights(self.handle, w.ctypes.data_as(C.c_void_p)))
        return w

    def cpu_frame_index(self):
        v = C.c_uint64()
        self._check(self.lib.plrf_get_cpu_frame_index(self.handle, C.byref(v)))
        return v.value


class SyntheticInputs:
    """everything the rasterised / out-of-scope passes would have produced, generated once per scene + camera"""

    def __init__(self, scene: synth.SynthScene, cam: Camera, cam_prev: Camera, width, height, sdf_res, shadow_res, froxel_depth, sun_direction, cascades=3,
                 rows=None, depth_range=None):
        """rows=(r0, r1): generate the per-pixel inputs for these rows only (band rendering); depth_range=(min, max) linear depth of
        the WHOLE frame then has to be given so that every band fits the same shadow cascades"""
        self.width, self.height, self.sdf_res, self.shadow_res = width, height, sdf_res, shadow_res
        self.rows = rows
        self.gb = scene.gbuffer(cam, width, height, cam_prev, rows=rows)
        self.instance_bytes, self.bb_bytes, self.volumes = scene.sdf_instances(sdf_res)
        self.noise = synth.blue_noise_standins()
        self.sky = synth.sky_lut()
        self.transmission = synth.transmission_lut()
        sun = np.asarray(sun_direction, np.float64)
        self.sun = sun / np.linalg.norm(sun)
        depth = self.gb["depth"]
        n, f = cam.near, cam.far
        vis = depth[depth > 0]
        lin = n * f / (f + (1.0 - vis.astype(np.float64)) * (n - f)) if vis.size else np.array([1.0, 50.0])
        self.depth_range = depth_range if depth_range is not None else (float(lin.min()), float(lin.max()))
        self.shadow_info, self.shadow_maps = scene.shadow_cascades(cam, self.sun, self.depth_range[0], self.depth_range[1], shadow_res, cascade_count=cascades)
        self.froxel, self.froxel_dims = synth.froxel_volume(width, height, froxel_depth)
        self.vol_settings = synth.volumetric_settings_bytes(30.0)

    # ---- fixtures: the generated arrays as a flat dict of numpy arrays and back (tests/golden)
    def to_arrays(self):
        d = {"dims": np.array([self.width, self.height, self.sdf_res, self.shadow_res], np.int64), "sun": np.asarray(self.sun, np.float64),
             "instance_bytes": np.frombuffer(self.instance_bytes, np.uint8), "bb_bytes": np.frombuffer(self.bb_bytes, np.uint8),
             "shadow_info": np.frombuffer(bytes(self.shadow_info), np.uint8), "vol_settings": np.frombuffer(bytes(self.vol_settings), np.uint8),
             "sky": self.sky, "transmission": self.transmission, "froxel": self.froxel, "froxel_dims": np.asarray(self.froxel_dims, np.int64),
             "n_volumes": np.array([len(self.volumes)], np.int64)}
        for k, v in self.gb.items():
            d["gb_" + k] = v
        for i, v in enumerate(self.volumes):
            d["volume_%d" % i] = v
        for i in range(4):
            d["shadow_map_%d" % i] = self.shadow_maps[i]
            d["noise_%d" % i] = self.noise[i]
        return d

    @classmethod
    def from_arrays(cls, d):
        self = cls.__new__(cls)
        self.width, self.height, self.sdf_res, self.shadow_res = (int(v) for v in d["dims"])
        self.sun = np.asarray(d["sun"], np.float64)
        self.instance_bytes, self.bb_bytes = d["instance_bytes"].tobytes(), d["bb_bytes"].tobytes()
        self.shadow_info, self.vol_settings = d["shadow_info"].tobytes(), d["vol_settings"].tobytes()
        self.sky, self.transmission, self.froxel = d["sky"], d["transmission"], d["froxel"]
        self.froxel_dims = tuple(int(v) for v in d["froxel_dims"])
        self.gb = {k[3:]: d[k] for k in d if k.startswith("gb_")}
        self.volumes = [d["volume_%d" % i] for i in range(int(d["n_volumes"][0]))]
        self.shadow_maps = [d["shadow_map_%d" % i] for i in range(4)]
        self.noise = [d["noise_%d" % i] for i in range(4)]
        return self

    def upload(self, fp: FramePipeline):
        be = fp.be
        gb = self.gb
        r0 = self.rows[0] if getattr(self, "rows", None) is not None else None
        up = (lambda img, a: be.uploadImageRows(img, r0, a)) if r0 is not None else be.uploadImage
        for i in (0, 1):
            up(fp.image("depth%d" % i), gb["depth"])
            up(fp.image("motion%d" % i), gb["motion"])
        up(fp.image("normal"), gb["normal"])
        up(fp.image("albedo"), gb["albedo"])
        up(fp.image("specular"), gb["specular"])
        be.uploadImage(fp.image("skyLut"), self.sky)
        be.uploadImage(fp.image("transmissionLut"), self.transmission)
        be.uploadImage(fp.image("volumetricIntegrationVolume"), self.froxel)
        for i in range(4):
            be.uploadImage(fp.image("shadow%d" % i), self.shadow_maps[i])
            be.uploadImage(fp.image("noise%d" % i), self.noise[i])
        be.setStorageBufferData(fp.storage_buffer("sunShadowInfo"), self.shadow_info)
        be.setUniformBufferData(fp.uniform_buffer("volumetricSettings"), self.vol_settings)
        self.volume_indices = [fp.add_sdf_volume(self.sdf_res, v) for v in self.volumes]
        inst = bytearray(self.instance_bytes)
        for i, ti in enumerate(self.volume_indices):
            struct.pack_into("<I", inst, 16 + i * 96 + 12, ti)
        self.instance_bytes_patched = bytes(inst)
        fp.set_sdf_scene(self.instance_bytes_patched, self.bb_bytes)
        fp.set_sun_direction(self.sun)
