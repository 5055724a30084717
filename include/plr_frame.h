/* plr_frame.h - C entry points of the C++ host-side frame pipeline (plainrenderer_amd/csrc/frontend/frame_pipeline.*).
 *
 * The pipeline is the compute part of the reference's RenderFrontend::prepareRenderpasses (RenderFrontend.cpp:313-406) and its
 * technique classes, recorded through the RenderBackend boundary of plr.h. These functions exist so a benchmark / test harness
 * in another language can drive whole frames; the reference itself would call the C++ classes directly.
 * plr_setup() must have been called first. All functions return PLR_OK or a negative code (message: plrf_last_error()).
 */
#ifndef PLR_FRAME_H
#define PLR_FRAME_H
#include "plr.h"
#include "plr_sdf_bake.h" /* plr_mesh_data */
#ifdef __cplusplus
extern "C" {
#endif

typedef struct plrf_settings {
    uint32_t width, height;
    uint32_t shadow_map_res;      /* 2048 in the reference (RenderFrontend.cpp:40) */
    uint32_t brdf_lut_res;        /* 512 (RenderFrontend.cpp:45) */
    uint32_t max_sdf_instances;   /* 1200 (SceneConfig.h:3) */
    uint32_t froxel_depth;        /* 64 */
    /* TAASettings, Techniques/TAA.h:8-17 */
    uint32_t taa_enabled, taa_use_clipping, taa_use_motion_vector_dilation, taa_history_sampling_tech, taa_filter_use_tonemapping;
    /* BloomSettings, Techniques/Bloom.h:5-9 */
    uint32_t bloom_enabled; float bloom_strength, bloom_radius;
    /* SDFTraceSettings, Techniques/SDFGI.h:17-29 */
    uint32_t sdf_half_res_trace, sdf_strict_influence_radius_cutoff; float sdf_trace_influence_radius;
    /* ShadingConfig, RenderFrontend.h:32-38 */
    uint32_t diffuse_brdf, direct_multiscatter, indirect_lighting_tech, use_geometry_aa, sun_shadow_cascade_count;
    /* which pass groups of the frame are recorded (all 1 = full frame) */
    uint32_t run_exposure, run_hiz, run_gi, run_shading, run_taa, run_bloom, run_tonemap;
    /* band rendering (multi-GPU partition by screen rows; no reference counterpart). width/height stay the whole frame's; this
     * instance renders full-resolution rows [band_row_begin, band_row_end) (multiples of 64, or the last row). band_row_end == 0:
     * off. Halos: rows exchanged / recomputed around the band, see BandSettings in csrc/frontend/frame_pipeline.h */
    uint32_t band_row_begin, band_row_end, band_gi_halo, band_gi_history_halo, band_color_halo, band_post_halo;
    /* band_gi_halo decides what a partitioned frame IS. The GI denoiser's disc is 1.5 m in world space - on near geometry wider than any bounded halo - and a
     * sample beyond the exchanged halo gets weight 0. The denoised signal is next frame's history (SDFGI.cpp:421-536), so that deviation feeds back and spreads:
     * with the default (64 trace rows per 2160 frame rows) the share of pixels more than one R11G11B10 code from the unpartitioned frame grows for hundreds of
     * frames and has no steady state within 256 (profiles/r05_config5_series.txt). band_gi_halo = PLRF_HALO_WHOLE_IMAGE exchanges every GI texel with every
     * rank: the partitioned frame then EQUALS the unpartitioned one, bit for bit (tests/test_config5_8k.py, 64 frames at 8K), at the price in the same file. */
#define PLRF_HALO_WHOLE_IMAGE 0xffffffffu
    /* band_gi_halo = PLRF_HALO_REQUESTED (round 6; half-resolution trace only): REQUEST LISTS instead of a halo in front of the two spatial filter passes. Where a disc
     * sample lands depends on depth, camera and frame index only (filterIndirectDiffuseSpatial.comp:53-105), so right after the depth downscale a giSampleRequests pass per
     * filter marks, in a bitmap over the trace image, every texel outside this rectangle a sample of this rectangle's pixels lands on; the exchange callback
     * PLRF_EXCHANGE_GI_REQUESTS trades the bitmaps (to each peer the part over its rectangle) while the trace runs, and at PLRF_EXCHANGE_GI_TRACE /
     * PLRF_EXCHANGE_GI_TEMPORAL every owner sends exactly the requested texels - Y_SH, CoCg and the half-resolution depth, 16 bytes each - which the receiver scatters
     * into its images. Nothing is masked, nothing is approximated: the partitioned frame EQUALS the unpartitioned one bit for bit (tests/test_config5_8k.py), like
     * PLRF_HALO_WHOLE_IMAGE, for 6 - 27 MB received per rank and frame at 8K instead of 200 MB (profiles/r06_gi_request_count.txt). plrf_get_gi_request_exchange
     * describes the buffers to an exchange callback; the native exchange (plrf_rccl_attach_rects / plrf_local_attach_rects) implements it. */
#define PLRF_HALO_REQUESTED 0xfffffffeu
    /* input producers recorded as compute passes instead of uploaded (0 = uploaded): lightMatrix.comp after the depth pyramid */
    uint32_t run_light_matrix; float volumetrics_max_distance;
    uint32_t taa_use_separate_supersampling, taa_supersample_use_tonemapping; /* TAASettings::useSeparateSupersampling (off), supersampleUseTonemapping */
    uint32_t sdf_debug_mode, sdf_debug_tile_usage_with_hiz, sdf_debug_use_influence_radius; /* SDFDebugSettings (SDFGI.h:9-15): mode != 0 replaces the frame by the debug view */
    uint32_t band_taa_history_halo; /* rows of the TAA history exchanged between bands (default 32) */
    uint32_t run_volumetrics; /* the four froxel passes produce volumetricIntegrationVolume (reference default VolumetricsSettings; noise volume "perlinNoise3D" is an input) */
    uint32_t run_sky_luts; /* sky transmission / multiscatter / sky LUT compute passes with the reference's default AtmosphereSettings */
    uint32_t band_overlap_exchange; /* 0: one call per exchange. 1: producers of exchanged images run their edge rows first and the exchange callback is called
                                       twice, with PLRF_EXCHANGE_BEGIN (start, do not wait) and PLRF_EXCHANGE_END (wait).
                                       2 (the default): as 1, but the producer is ONE launch that writes the edge rows first and raises plr_get_edge_signal when they
                                       are complete (plr.h first_rows) - the BEGIN callback may wait for that signal on its own stream instead of ordering
                                       behind the launch stream; 1: an edge launch and an interior launch with the BEGIN callback between them (round 3) */
    /* tile rendering (round 5; BASELINE config 5: the frame as 2 x 2 screen tiles over 4 GPUs): this instance renders columns [band_col_begin, band_col_end) of
     * its rows (multiples of 64, or the last column). band_col_end == 0: whole rows (a band). The halos are the same numbers of columns; exchange items then
     * carry a column range and the transfers are rectangles (plrf_exchange_plan_rects). With band_overlap_exchange 1 a tile behaves as with 0 (its producers
     * are never split); 2 produces the FRAME of the tile first (plr.h first_rows + first_cols). */
    uint32_t band_col_begin, band_col_end;
    /* 1: a partitioned pipeline (band_row_end or band_col_end non-zero) rasterises scene meshes and shadow casters: the eight scene / caster calls below behave
     * as on an unpartitioned pipeline (same validation, lifetime and removal rules). The depth prepass is recorded with the 44-byte pass record, restricted to this
     * rank's raster window (plrf_raster_window_for): the tiles of the owned rectangle and of everything a pass of this pipeline reads around it. G-buffer texels
     * outside the window and its wrap strips (plrf_raster_wrap_strips_for) are never written and never read. Every rank rasterises every shadow cascade in full: the maps are not screen-partitioned (the redundancy
     * is inherent, like the bloom chain's), and with run_light_matrix their matrices come from the all-reduced depth range, so all ranks draw the same maps.
     * plrf_get_prepass_raster_stats does not depend on the window. 0 (the default): those calls are refused with PLR_ERR_UNSUPPORTED on a partitioned pipeline and the
     * G-buffer is uploaded. No effect on an unpartitioned pipeline. Fixed for the pipeline's lifetime, like the other band fields. (It stands with the band fields, in
     * front of run_sky, which stays the struct's last field.) */
    uint32_t band_raster;
    /* 1: "skyAndSunSprite.comp" right after the deferred shade (Sky::renderSky, Techniques/Sky.cpp:318-353, as one compute pass over the depth == 0 pixels of
     * the colour buffer: the banding dither, the froxel in-scattering on the sky and the sun disc with limb darkening; geometry pixels are not touched). Off by
     * default. Needs run_shading (plrf_create: PLR_ERR_INVALID_ARGUMENT otherwise), is not recorded while sdf_debug_mode != 0 and is fixed for the pipeline's
     * lifetime like the other run_* flags. */
    uint32_t run_sky;
} plrf_settings;

/* The raster window of a pipeline with these settings, in 64 x 64 tiles of the frame, half-open: out_tiles = {x0, y0, x1, y1}. It is the owned rectangle grown, on
 * every side that has a neighbour, by the largest reach with which a pass of the pipeline reads the G-buffer images outside the rectangle (DESIGN.md "Rasterising
 * in a partition" derives it pass by pass), rounded out to whole tiles and clipped to the frame; the whole grid for an unpartitioned frame and for whole-image halos.
 * A pure host function: no backend call, valid without a GPU. It does not depend on band_raster. */
int plrf_raster_window_for(const plrf_settings* settings, uint32_t out_tiles[4]);
/* The wrap strips of that window: out_tiles receives *out_count (0 .. 3) more tile rectangles, four words each. The temporal GI filter reads last frame's motion with
 * repeat addressing, so from a window that touches a frame edge without spanning the frame it reaches the tile column / row at the OPPOSITE edge; a partition
 * rasterises those tiles too, one more execution of the pass per strip. Outside the window and its strips no G-buffer texel is written or read. */
int plrf_raster_wrap_strips_for(const plrf_settings* settings, uint32_t out_tiles[12], uint32_t* out_count);
/* the same for a pipeline's current settings: the window its depth prepass is recorded with when band_raster is 1 */
int plrf_get_raster_window(void* pipeline, uint32_t out_tiles[4]);

/* ---- band rendering: halo exchange hooks ----
 * While plrf_frame launches the passes it calls the exchange callback, in pass order, at the points where rows produced by
 * neighbouring bands are needed. The callback moves the rows (RCCL send/recv on the stream it is handed, or any other transport)
 * of every item plrf_get_exchange_items reports for that exchange id; PLRF_EXCHANGE_HISTOGRAM instead sums the 128-bin luminance
 * histogram over all bands in place (plrf_get_histogram_exchange). */
enum plrf_exchange_id { PLRF_EXCHANGE_HISTOGRAM = 0, PLRF_EXCHANGE_GI_TRACE = 1, PLRF_EXCHANGE_GI_TEMPORAL = 2, PLRF_EXCHANGE_GI_HISTORY = 3,
                        PLRF_EXCHANGE_POST = 4,
                        /* only with run_light_matrix: the depth range of the whole frame for the cascade fit (lightMatrix.comp:76-78 reads the apex of the
                         * depth pyramid; a band has none). plrf_get_depth_apex_exchange names two floats {min, max} in device memory holding the band's
                         * range: replace them IN PLACE by the minimum of all bands' first and the maximum of all bands' second float (exact: the result
                         * equals the unpartitioned pyramid's apex bit for bit) */
                        PLRF_EXCHANGE_DEPTH_APEX = 5, PLRF_EXCHANGE_GI_REQUESTS = 6, PLRF_EXCHANGE_COUNT = 7 };
/* phase bits or-ed into exchange_id when band_overlap_exchange is on (ids 1..4; the histogram is always one call): after the producer's
 * edge rows are launched the callback gets id | PLRF_EXCHANGE_BEGIN and must only START the transfers (stream-ordered after what is already
 * on hip_stream); the producer's interior rows are launched next and run beside the transfers; before the first consumer of the halo rows
 * the callback gets id | PLRF_EXCHANGE_END and must make hip_stream wait for their completion. No bits: start and wait in one call. */
enum plrf_exchange_phase { PLRF_EXCHANGE_BEGIN = 0x100, PLRF_EXCHANGE_END = 0x200, PLRF_EXCHANGE_ID_MASK = 0xff };
typedef int (*plrf_exchange_callback)(void* user, int exchange_id, void* hip_stream);
/* an image of image_rows rows of row_bytes bytes at device_ptr; this band owns rows [row_begin, row_end): it sends its first
 * halo_rows owned rows to the band above and its last halo_rows to the band below, and receives rows
 * [row_begin - halo_rows, row_begin) from above and [row_end, row_end + halo_rows) from below (clipped to the image) */
typedef struct plrf_exchange_item {
    plr_image_handle image;
    void* device_ptr;
    uint32_t row_begin, row_end, halo_rows, row_bytes, image_rows;
    /* tile rendering: the rectangle this instance owns is columns [col_begin, col_end) of those rows, of an image of image_cols texels of texel_bytes bytes per row
     * (a band: 0 .. image_cols); the halo is halo_rows texels on every side that has a neighbour, corners included */
    uint32_t col_begin, col_end, image_cols, texel_bytes;
} plrf_exchange_item;
int plrf_set_exchange_callback(void* pipeline, plrf_exchange_callback callback, void* user);
/* items of the frame being launched (valid inside the callback and until the next plrf_frame); *inout_count = capacity in, count out */
int plrf_get_exchange_items(void* pipeline, int exchange_id, plrf_exchange_item* out_items, uint32_t* inout_count);
int plrf_get_histogram_exchange(void* pipeline, void** out_device_ptr, size_t* out_bytes);
/* the request-list exchange (band_gi_halo = PLRF_HALO_REQUESTED): the trace image's size, this rank's rectangle in trace texels, and per spatial filter pass (0: its
 * input is the traced GI, exchanged at PLRF_EXCHANGE_GI_TRACE; 1: the temporally filtered GI, PLRF_EXCHANGE_GI_TEMPORAL) the request bitmap (row_words 32-bit words
 * per texel row; bit x % 32 of word x / 32) and the input images; depth = the filters' R16F depth texture. enabled = 0: the pipeline does not use request lists. */
typedef struct plrf_gi_request {
    int32_t enabled;
    uint32_t image_cols, image_rows, row_words;
    uint32_t x0, y0, x1, y1;
    void* bitmap[2];
    void* ysh[2];
    void* cocg[2];
    void* depth;
} plrf_gi_request;
int plrf_get_gi_request_exchange(void* pipeline, plrf_gi_request* out);
/* non-zero: this pipeline records rows-first producers (band_overlap_exchange 2): a BEGIN callback may wait for plr_get_edge_signal */
int plrf_band_rows_first(void* pipeline);
int plrf_get_depth_apex_exchange(void* pipeline, void** out_device_ptr, size_t* out_bytes); /* 8 bytes: float min, float max */

/* ---- the same exchange, natively over RCCL (csrc/frontend/band_exchange.cpp): one process per GPU, one band per process ----
 * plrf_rccl_attach creates this rank's communicator (ncclCommInitRank with the id rank 0 obtained from plrf_rccl_get_unique_id and handed to
 * every rank by the launcher, once) and installs a C++ exchange callback on the pipeline: per exchange one group of ncclSend / ncclRecv with
 * the band above and the band below on a communication stream ordered against the launch stream by events (BEGIN / END phases), and one
 * 512-byte ncclAllReduce for the luminance histogram. frame_height = rows of the whole frame (bands = plrf_band_rows of it). */
#define PLRF_RCCL_UNIQUE_ID_BYTES 128
int plrf_rccl_get_unique_id(void* out_128_bytes);
int plrf_rccl_attach(void* pipeline, const void* unique_id_128_bytes, int rank, int world, uint32_t frame_height, void** out_exchange);
/* the same for a partition chosen by the caller (load balancing: bands of unequal height): row_bounds = world + 1 row boundaries, 0 ... frame_height,
 * interior ones multiples of 64; band r owns rows [row_bounds[r], row_bounds[r + 1]) and must have been created with exactly those rows. NULL = plrf_band_rows */
int plrf_rccl_attach_rows(void* pipeline, const void* unique_id_128_bytes, int rank, int world, uint32_t frame_height, const uint32_t* row_bounds, void** out_exchange);
int plrf_rccl_detach(void* pipeline, void* exchange);
/* bytes this rank sent / received and the number of point-to-point exchange groups of the last frame */
int plrf_rccl_get_stats(void* exchange, uint64_t* out_bytes_sent, uint64_t* out_bytes_received, uint64_t* out_exchanges);
/* single-GPU check of the transport: rows [src_row, src_row + rows) of an image are sent to and received from this rank itself onto
 * rows [dst_row, ...) through the same group / stream / event sequence as an overlapped exchange */
int plrf_rccl_self_test(void* exchange, void* device_ptr, uint32_t row_bytes, uint32_t src_row, uint32_t dst_row, uint32_t rows, void* launch_stream);
const char* plrf_rccl_last_error(void);
/* the partition and the per-item transfer plan the exchange uses (pure functions, no GPU): band `band` of `n_bands` owns full-resolution rows
 * [begin, end), multiples of 64; for one exchange item (an image of image_rows rows showing the frame at frame_height / image_rows scale, of
 * which this band owns [row_begin, row_end)) the plan lists up to 4 transfers: send / receive with the band above and below */
typedef struct plrf_exchange_op { uint32_t peer, send, row_begin, row_end; } plrf_exchange_op;
int plrf_band_rows(uint32_t frame_height, uint32_t n_bands, uint32_t band, uint32_t* out_row_begin, uint32_t* out_row_end);
int plrf_exchange_plan_rows(uint32_t frame_height, uint32_t n_bands, const uint32_t* row_bounds, uint32_t band, uint32_t image_rows, uint32_t halo_rows, uint32_t row_begin,
                            uint32_t row_end, plrf_exchange_op* out_ops, uint32_t* out_count);
/* what the native exchange moves for a band (up to 2 (n_bands - 1) transfers, out_count = how many there are): the plan above, plus - when a halo is taller
 * than a neighbouring band (band_gi_halo = PLRF_HALO_WHOLE_IMAGE) - the rows of the bands behind the neighbours */
int plrf_exchange_plan_all_bands(uint32_t frame_height, uint32_t n_bands, const uint32_t* row_bounds, uint32_t band, uint32_t image_rows, uint32_t halo_rows, uint32_t row_begin,
                                 uint32_t row_end, plrf_exchange_op* out_ops, uint32_t capacity, uint32_t* out_count);
int plrf_exchange_plan(uint32_t frame_height, uint32_t n_bands, uint32_t band, uint32_t image_rows, uint32_t halo_rows, uint32_t row_begin, uint32_t row_end,
                       plrf_exchange_op* out_ops_4, uint32_t* out_count);

/* ---- tile rendering (round 5): the partition is a list of pixel rectangles, one per rank (rects = world x {x0, y0, x1, y1} at full resolution; edges between
 * rectangles on multiples of 64). A band partition is the special case of full-width rectangles, and for it the plan below equals plrf_exchange_plan_rows.
 * For one exchange item (an image of image_cols x image_rows texels showing the frame at frame_width / image_cols scale) rank `rank` exchanges with every
 * rank whose rectangle TOUCHES its own (shares an edge or a corner - on a 2 x 2 grid all three others; xGMI connects every pair of GPUs of a node directly, so the
 * diagonal neighbour is one more peer of the same group, not a second hop): it sends the part of its own rectangle that lies within halo texels of the peer's
 * and receives the part of the peer's that lies within halo texels of its own (corners included). Ops are listed by ascending peer, send before receive;
 * capacity = 2 x (world - 1) covers every case. */
typedef struct plrf_rect_op { uint32_t peer, send, x0, y0, x1, y1; } plrf_rect_op;
int plrf_exchange_plan_rects(uint32_t frame_width, uint32_t frame_height, uint32_t world, const uint32_t* rects, uint32_t rank, uint32_t image_cols, uint32_t image_rows,
                             uint32_t halo, plrf_rect_op* out_ops, uint32_t capacity, uint32_t* out_count);
/* gx x gy grid of tiles over the frame, row-major (rank = ty * gx + tx), every edge a multiple of 64; col_bounds (gx + 1) / row_bounds (gy + 1) choose the cuts
 * (load balancing), NULL = equal parts. out_rects: gx * gy * 4 values */
int plrf_tile_rects(uint32_t frame_width, uint32_t frame_height, uint32_t gx, uint32_t gy, const uint32_t* col_bounds, const uint32_t* row_bounds, uint32_t* out_rects);
/* the native exchange for a partition into rectangles: as plrf_rccl_attach_rows, but rank r owns rects[4 r .. 4 r + 3] and must have been created with exactly that
 * rectangle (band_row_* / band_col_*). Rectangles that are not whole rows are moved through staging buffers: ONE pack kernel gathers every region of every image
 * of the exchange point for all peers, one group of ncclSend / ncclRecv (one pair per peer) moves the buffers, ONE unpack kernel scatters what arrived.
 * unique_id_128_bytes == NULL: LOOPBACK - no communicator; pack, a device copy standing in for the links, unpack, on the same streams and events (what a
 * single-GPU replay of a partition's frame costs, tools/band_cost.py; the received texels are meaningless). */
int plrf_rccl_attach_rects(void* pipeline, const void* unique_id_128_bytes, int rank, int world, uint32_t frame_width, uint32_t frame_height, const uint32_t* rects,
                           void** out_exchange);
/* ---- the IN-PROCESS transport (round 6): every rank of the partition in ONE process on one GPU - one host thread, backend, pipeline and exchange each, as the
 * partition tests run them. The exchange is the communicator path's code (plans, pack / unpack kernels, communication stream, BEGIN behind the producers' edge
 * signal, END, watchdog); where ncclSend / ncclRecv go, a rank publishes its transfers with an event behind its pack, waits on the host until its peers have posted
 * the same exchange, copies their send ranges into its receive ranges on its own stream (the k-th send of a to b pairs with b's k-th receive from a, RCCL's rule
 * inside a group) and orders its stream behind the peers' reads of what it sent. The all-reduces go through slots of group memory. One group per partition; it
 * must outlive its exchanges (plrf_rccl_detach). plrf_local_group_abort: wake ranks waiting for a peer that failed. plrf_local_group_freeze(1): a rank no longer
 * waits for its peers and copies from what they posted LAST (their buffers keep their last frame's texels): tools/band_cost.py times ONE partition alone with real
 * neighbour data in its halos. */
int plrf_local_group_create(int world, void** out_group);
int plrf_local_group_destroy(void* group);
int plrf_local_group_abort(void* group);
int plrf_local_group_freeze(void* group, int frozen);
int plrf_local_attach_rects(void* pipeline, void* group, int rank, int world, uint32_t frame_width, uint32_t frame_height, const uint32_t* rects, void** out_exchange);
/* what the exchange runs on: ranks of the communicator (ncclCommCount; 0 in loopback), the RCCL version code (ncclGetVersion), the ordering mode of the overlapped
 * exchanges (2 = the producer's edge signal + hipStreamWaitValue32, 1 = an event behind the producer - also what mode 2 falls back to on a device without
 * stream memory operations, 0 = not overlapped), whether the regions go through pack / unpack kernels (a tile partition) or straight from the images (bands) */
typedef struct plrf_rccl_info { int32_t rccl_ranks, rccl_version, overlap_mode, packed_regions, stream_wait_value_supported, watchdog_ms; } plrf_rccl_info;
int plrf_rccl_get_info(void* exchange, plrf_rccl_info* out);
/* single-GPU check of the pack / unpack kernels and the packed transport: the rectangle [x0, x1) x [y0, y1) (texels of texel_bytes bytes) of an image of pitch_bytes
 * per row goes through pack -> ncclSend / ncclRecv with this rank as its own peer (loopback: a device copy) -> unpack onto the rectangle of the same size at (dst_x, dst_y) */
int plrf_rccl_self_test_rect(void* exchange, void* device_ptr, uint32_t pitch_bytes, uint32_t texel_bytes, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t dst_x,
                             uint32_t dst_y, void* launch_stream);

/* ---- exchange watchdog (round 5): an overlapped exchange is a wait the launch stream parks on; if a peer never posts its side the frame
 * hangs and says nothing. Every BEGIN arms an entry {rank, exchange id, phase, completion query, time}; entries are checked at every later exchange
 * callback (the frame then fails with the message) and by a background thread every 50 ms, which prints the message to stderr when an entry goes overdue - a REPORT:
 * a peer paused in a debugger or an oversubscribed host recovers, and the thread says so and frames go on (round 6) - and aborts the process only when
 * the entry is still incomplete PLRF_EXCHANGE_WATCHDOG_ABORT_MS later (default 30000; PLRF_EXCHANGE_WATCHDOG_ABORT=0: never): a hung collective cannot be
 * cancelled, only reported. Deadline: PLRF_EXCHANGE_WATCHDOG_MS (default 2000, 0 = off); the first 64 exchanges of a communicator (about ten frames: RCCL sets up its point-to-point connections inside the first group with each peer, and ranks
 * leave their set-up at different times) get PLRF_EXCHANGE_WATCHDOG_FIRST_MS (default 60000) instead. The functions below expose the mechanism with a caller-supplied completion query, so it can be tested without a GPU. */
typedef int (*plrf_watchdog_query)(void* user); /* 0 = still running, 1 = complete */
int plrf_watchdog_create(uint32_t deadline_ms, void** out_watchdog);
int plrf_watchdog_destroy(void* watchdog);
int plrf_watchdog_arm(void* watchdog, int rank, int exchange_id, int phase, plrf_watchdog_query query, void* user);
/* 0: nothing overdue (completed entries are dropped); 1: an entry is past its deadline - out_message names rank, exchange and phase */
int plrf_watchdog_poll(void* watchdog, char* out_message, size_t capacity);

typedef struct plrf_camera { float position[3], forward[3], up[3], right[3]; } plrf_camera;

int plrf_default_settings(plrf_settings* out, uint32_t width, uint32_t height);
int plrf_create(const plrf_settings* settings, void** out_pipeline);
int plrf_destroy(void* pipeline);
const char* plrf_last_error(void);
/* named resources: see FramePipeline::image / storageBuffer / uniformBuffer */
int plrf_get_image(void* pipeline, const char* name, plr_image_handle* out);
int plrf_get_storage_buffer(void* pipeline, const char* name, plr_storage_buffer_handle* out);
int plrf_get_uniform_buffer(void* pipeline, const char* name, plr_uniform_buffer_handle* out);
/* registers one R16F res^3 SDF volume, returns its global texture array index (SDFInstance.sdfTextureIndex) */
int plrf_add_sdf_volume(void* pipeline, uint32_t res, const void* half_data, size_t bytes, uint32_t* out_texture_index);
/* the same from a DDS file written by the asset pipeline (plr_write_dds_file / the reference's writeDDSFile): any width x height x depth */
int plrf_add_sdf_volume_dds(void* pipeline, const char* path, uint32_t* out_texture_index, uint32_t out_size[3]);
/* {uint count; uint pad[3]; SDFInstance[count]} and {vec3 min; float; vec3 max; float}[count] (SDFGI::updateSDFScene). While a scene SDF is set
 * (plrf_set_scene_sdf below) the pipeline writes both buffers itself every frame: the call then returns PLR_ERR_UNSUPPORTED and changes nothing. After the scene
 * SDF was removed the instance count is 0 until the caller uploads again. */
int plrf_set_sdf_scene(void* pipeline, const void* instance_buffer, size_t instance_bytes, const void* world_bbs, size_t bb_bytes);
int plrf_set_sun_direction(void* pipeline, const float direction[3]);
int plrf_set_camera_intrinsic(void* pipeline, float fov_degrees, float near_plane, float far_plane);
int plrf_set_camera_cut(void* pipeline);
/* ---- live changes (RenderFrontend::setResolution, RenderFrontend.cpp:408-421, and the stale-flag branches of prepareNewFrame, :198-278): both calls only RECORD
 * the change; it is applied at the start of the next plrf_frame, before the passes are recorded, or by plrf_apply_changes.
 * plrf_set_resolution: every image and buffer whose size follows the screen (render targets, post-process buffers, TAA history, GI images at trace resolution and
 * the upscale targets, HiZ pyramid, half-resolution depth, froxel volumes, swapchain, per-tile histogram, culled tiles) is re-created zero-filled, as plrf_create
 * creates it, and the next frame is a camera cut; a resize to the size the images already have keeps them (only the cut). What survives: the light buffer
 * (exposure), the frame counters and the TAA jitter position, SDF volumes and scene, sun direction, camera intrinsics but the aspect ratio, BRDF LUT, shadow maps,
 * sky LUTs, noise textures. Inputs that follow the screen (G-buffer, and the froxel volume when run_volumetrics is 0) are the caller's to upload again.
 * Width or height 0 = minimized (RenderFrontend.cpp:229): plrf_frame returns PLR_OK, records and launches nothing, counts nothing; the next non-zero size
 * resumes with a camera cut.
 * plrf_update_settings: the settings the reference's UI edits (:1882-2011) - taa_*, bloom_*, sdf_half_res_trace, sdf_strict_influence_radius_cutoff,
 * sdf_trace_influence_radius, diffuse_brdf, direct_multiscatter, indirect_lighting_tech, use_geometry_aa, sdf_debug_*. A diffuse_brdf change re-bakes the BRDF LUT,
 * a trace-resolution change re-creates the GI images (zero-filled) and cuts, a TAA change updates the pass descriptions only. Any other field that differs from
 * the pipeline's returns PLR_ERR_UNSUPPORTED, a width / height other than the current resolution PLR_ERR_INVALID_ARGUMENT; the pipeline is then untouched.
 * Partitioned pipelines (band_row_end or band_col_end non-zero) refuse both calls with PLR_ERR_UNSUPPORTED: the exchange plan and an attached exchange follow
 * the frame size, and re-partitioning a live frame is out of scope. */
int plrf_set_resolution(void* pipeline, uint32_t width, uint32_t height);
int plrf_update_settings(void* pipeline, const plrf_settings* settings);
int plrf_apply_changes(void* pipeline); /* apply what was recorded now: a caller uploads the new size's inputs after it */
/* ---- mesh shadow casters: RenderFrontend::renderSunShadowCascades (RenderFrontend.cpp:354, 760-774) as the compute pass "sunShadowRaster.comp".
 * While a pipeline has casters, every plrf_frame records sun_shadow_cascade_count executions of the pass behind the light matrices (also under sdf_debug_mode);
 * they rasterise the draws into shadow0 .. shadow<count - 1> with whatever sunShadowInfo holds, uploaded or computed (run_light_matrix). Maps at and above the
 * cascade count are not touched. Without casters nothing is recorded and the uploaded maps are used. The rasterisation contract - 8 sub-pixel bits, top-left
 * rule, front faces culled, depth clamp, round-to-nearest-even Depth16, a 2^20-pixel guard band with a counted reject instead of clipping, casters opaque unless
 * plrf_set_shadow_caster_cutouts or plrf_set_shadow_caster_cutouts_formatted (below) gives them an alpha test - is DESIGN.md "Sun shadow cascades as a compute pass".
 * plrf_set_shadow_casters copies the meshes (positions and a uint32 triangle list each) and the draws; draw_count 0 removes the casters. PLR_ERR_INVALID_ARGUMENT,
 * with a message that names the cause: a mesh index or a vertex index out of range, an index count that is no multiple of 3, a model matrix whose last row is not
 * exactly (0, 0, 0, 1) (the pass does not divide by w). PLR_ERR_UNSUPPORTED: a band / tile pipeline without band_raster. A refused call changes nothing.
 * plrf_set_shadow_caster_transforms replaces the draws' model matrices (draw_count x 16 floats) from the next frame on, like setStorageBufferData: queued, applied
 * in call order; a draw_count other than the casters' is PLR_ERR_INVALID_ARGUMENT.
 * plrf_get_shadow_raster_stats: the counters of the last frame's execution for one cascade; waits for the GPU. submitted = triangles of all draws, drawn = back
 * faces inside the guard band whose pixel box meets the map, guard_band_rejects = triangles with a non-finite or out-of-band vertex. While
 * plrf_set_draw_culling has PLRF_CULL_SHADOW_CASTERS set, the three counters count the draws the cull kept for that cascade only. */
typedef struct plrf_shadow_draw { uint32_t mesh; float model_matrix[16]; } plrf_shadow_draw; /* glm column-major */
int plrf_set_shadow_casters(void* pipeline, const plr_mesh_data* meshes, uint32_t mesh_count, const plrf_shadow_draw* draws, uint32_t draw_count);
int plrf_set_shadow_caster_transforms(void* pipeline, const float* matrices16, uint32_t draw_count);
typedef struct plrf_shadow_raster_stats { uint64_t triangles_submitted, triangles_drawn, guard_band_rejects; } plrf_shadow_raster_stats;
int plrf_get_shadow_raster_stats(void* pipeline, uint32_t cascade, plrf_shadow_raster_stats* out);
/* ---- scene meshes: RenderFrontend::renderDepthPrepass (RenderFrontend.cpp:351, 792-802) as the compute pass "depthPrepassRaster.comp".
 * While a pipeline has a scene, every plrf_frame records one execution of the pass in front of the light matrices and the depth pyramid (also under
 * sdf_debug_mode). It rasterises the draws with the pipeline's own jittered viewProjection into the CURRENT frame's depth<i> and motion<i> and into normal, albedo
 * and specular, and writes every texel of the five images (depth 0 = sky where nothing is drawn); what the caller uploaded to them is overwritten, and a resize
 * needs no re-upload of the G-buffer. Without a scene nothing is recorded, created or allocated and the uploaded G-buffer is used. The rasterisation contract -
 * Sutherland-Hodgman clipping against the near plane and a 32-NDC guard volume, 8 sub-pixel bits, top-left rule, back faces culled with a counter-clockwise front
 * face, reverse-Z Depth32 with GreaterEqual and the later triangle winning a tie, perspective-correct fp64 attributes, opaque meshes, one constant material per
 * draw unless plrf_set_scene_textures (below) gives it textures - is DESIGN.md "Depth prepass as a compute pass".
 * plrf_scene_mesh: positions and optional normals (3 floats per vertex; NULL, or a vertex normal of exactly (0, 0, 0): the triangle's face normal
 * normalize(cross(v0 - v2, v0 - v1)) of the model-space positions) and a uint32 triangle list. plrf_scene_draw: a mesh under a model matrix with the two RGBA8
 * texels (R in the low byte) every pixel of the draw stores to albedo and specular.
 * plrf_set_scene_meshes copies everything; draw_count 0 removes the scene and the uploaded G-buffer is used again. PLR_ERR_INVALID_ARGUMENT, with a message that
 * names the cause: a mesh index or a vertex index out of range, an index count that is no multiple of 3, a non-finite matrix element. PLR_ERR_UNSUPPORTED: a
 * band / tile pipeline without band_raster, for every call, a removal (draw_count 0) included - it could only be a no-op there. A refused call changes nothing.
 * plrf_set_scene_mesh_transforms replaces the draws' model matrices (draw_count x 16 floats) from the next frame on; a draw_count other than the scene's is
 * PLR_ERR_INVALID_ARGUMENT. A draw's previous model matrix (motion vectors) is the one the last recorded frame used; on the first frame after
 * plrf_set_scene_meshes and after a camera cut it equals the current one.
 * plrf_get_prepass_raster_stats: the counters of the last frame's execution for the scene now set; waits for the GPU. All zero while no scene is set (also after a
 * removal) and before the first frame of a newly set scene. submitted = triangles of all draws, clipped = triangles the clip
 * changed, subtriangles_drawn = front-facing sub-triangles whose pixel box meets the frame, rejects = triangles outside their buffers or with a non-finite clip
 * coordinate plus sub-triangles with a vertex w <= 0 or outside the 2^20-pixel band. The storage buffer "mainPassMatrices" (plrf_get_storage_buffer) holds the
 * {model, mvp, mvpPrevious} the last frame wrote, 48 floats per draw. While plrf_set_draw_culling has PLRF_CULL_SCENE set, the four counters count the draws the
 * cull kept only. */
typedef struct plrf_scene_mesh { const float* positions; const float* normals; uint32_t vertex_count; const uint32_t* indices; uint32_t index_count; } plrf_scene_mesh;
typedef struct plrf_scene_draw { uint32_t mesh; float model_matrix[16]; uint32_t albedo_rgba8, specular_rgba8; } plrf_scene_draw; /* glm column-major */
int plrf_set_scene_meshes(void* pipeline, const plrf_scene_mesh* meshes, uint32_t mesh_count, const plrf_scene_draw* draws, uint32_t draw_count);
int plrf_set_scene_mesh_transforms(void* pipeline, const float* matrices16, uint32_t draw_count);
/* ---- material textures of the scene meshes: depthPrepass.frag / triangle.frag's albedoTexture and specularTexture sampled per pixel with the interpolated UV and
 * g_mipBias (DESIGN.md "Material textures in the depth prepass": the sampling contract in integers and IEEE operations - repeat addressing, isotropic trilinear
 * filtering with 8 sub-texel and 8 level-fraction bits, forward-difference derivatives of the triangle's own plane, round half even; the alpha test: plrf_set_scene_alpha_cutoffs below; the normal map: plrf_set_scene_normal_maps below; anisotropic filtering in place of the isotropic: plrf_set_scene_anisotropy below).
 * plrf_scene_texture: RGBA8 texels, R in the low byte, row-major; mip_count >= 1: that many levels back to back, level l being max(1, width >> l) x
 * max(1, height >> l); mip_count 0: level 0 only and the host builds the full chain, each texel the rounded mean (a + b + c + d + 2) >> 2 of the level below at
 * (min(2x, W - 1) | min(2x + 1, W - 1), min(2y, H - 1) | min(2y + 1, H - 1)). plrf_scene_material, one per draw: the texture an output samples, or PLRF_NO_TEXTURE
 * for the draw's constant albedo_rgba8 / specular_rgba8 word. mesh_uvs[k]: 2 floats per vertex of mesh k, NULL (the array or an entry): all (0, 0).
 * plrf_set_scene_textures needs a scene; mesh_count and draw_count must be the scene's. Everything is copied and takes effect with the next frame, in call order.
 * texture_count 0 removes textures and materials (the other arguments are not looked at), and so does every plrf_set_scene_meshes; they survive
 * plrf_set_scene_mesh_transforms, plrf_set_resolution and plrf_update_settings. Visibility, depth, motion, normal and the counters never depend on textures.
 * PLR_ERR_INVALID_ARGUMENT, with a message that names the cause: no scene set, a count mismatch, a texture size of 0 or above 16384, too many mips for the size,
 * NULL texels, a material index that is neither PLRF_NO_TEXTURE nor < texture_count, more than 2^28 texels in total, a non-finite UV. PLR_ERR_UNSUPPORTED: a band /
 * tile pipeline without band_raster. A refused call changes nothing. */
#define PLRF_NO_TEXTURE 0xffffffffu
typedef struct plrf_scene_texture { const uint32_t* texels; uint32_t width, height, mip_count; } plrf_scene_texture;
typedef struct plrf_scene_material { uint32_t albedo_texture, specular_texture; } plrf_scene_material;
int plrf_set_scene_textures(void* pipeline, const plrf_scene_texture* textures, uint32_t texture_count, const float* const* mesh_uvs, uint32_t mesh_count,
                            const plrf_scene_material* materials, uint32_t draw_count);
/* ---- block-compressed material textures (DESIGN.md "Block-compressed textures in the depth prepass"): plrf_set_scene_textures for textures that carry a format.
 * plrf_scene_texture_data: `data` holds `bytes` bytes. format PLR_FORMAT_RGBA8: the texels of a plrf_scene_texture, and the entry behaves exactly as one
 * (mip_count 0: the host builds the chain). format PLR_FORMAT_BC1, PLR_FORMAT_BC3 or PLR_FORMAT_BC5: the blocks of mip_count >= 1 levels back to back, level l being
 * ceil(W_l / 4) x ceil(H_l / 4) blocks (8 bytes for BC1, 16 for BC3 and BC5), row-major, with W_l = max(1, width >> l) - the payload of a DXT1 / DXT5 / ATI2 DDS
 * file as plr_load_dds_file returns it. The pass decodes the four taps of every footprint in integers (BC1: (r, g, b, 255), the BC1_RGB variant; BC3: (r, g, b, a),
 * the colour block always in four-colour mode; BC5: (R, G, 0, 255)) and then filters them as the sampling contract filters RGBA8 words; plr_decode_bc_to_rgba8
 * (plr_image_io.h) is the same decode on the host. `bytes` must be the exact size of the entry's levels. Semantics, lifetime and removal are
 * plrf_set_scene_textures': the stores replace one another, texture_count 0 removes, and alpha cutoffs and normal maps set afterwards index this store. A call whose
 * entries are all RGBA8 records exactly the pass plrf_set_scene_textures records. PLR_ERR_INVALID_ARGUMENT, with a message that names the cause: what
 * plrf_set_scene_textures refuses, an unknown format, mip_count 0 on a compressed entry, a bytes mismatch, more than 2^28 words in total (a compressed entry starts
 * at a multiple of 16 bytes). PLR_ERR_UNSUPPORTED: a band / tile pipeline without band_raster. A refused call changes nothing. */
typedef struct plrf_scene_texture_data {
    const void* data;
    uint64_t bytes;
    uint32_t width, height, mip_count, format; /* PLR_FORMAT_RGBA8 | BC1 | BC3 | BC5 */
} plrf_scene_texture_data;
int plrf_set_scene_textures_formatted(void* pipeline, const plrf_scene_texture_data* textures, uint32_t texture_count, const float* const* mesh_uvs, uint32_t mesh_count,
                                      const plrf_scene_material* materials, uint32_t draw_count);
/* ---- the texture store built on the GPU (DESIGN.md "Texture store built on the GPU": the chain, block gathering, colour block and alpha block contracts in
 * integers): plrf_set_scene_textures_formatted for a caller that holds level 0, or RGBA8 texels it wants stored compressed. plrf_scene_texture_source is a
 * plrf_scene_texture_data with the format the store is to hold. format RGBA8, store_format RGBA8: the levels as given, or with mip_count 0 level 0 and the GPU
 * builds the chain by the rule given above for plrf_scene_texture, byte for byte the host's chain. format RGBA8, store_format BC1 / BC3 / BC5: every level - given, or built -
 * is encoded on the GPU by the range-fit encode contract (BC1 ignores alpha, BC5 takes r and g). format BC1 / BC3 / BC5 with the same store_format: the levels as
 * given, or with mip_count 0 the blocks of level 0, which are kept verbatim, and levels 1 .. are decode(level 0), the chain rule, encode. Every other pair is refused;
 * the message names the texture and both formats. The store - table, formats, words - has exactly the layout plrf_set_scene_textures_formatted gives the same
 * textures with all their levels supplied (a compressed entry at a multiple of 4 words, no format buffer for an all-RGBA8 store). The RGBA8 staging chains the
 * build needs (every level of an entry that is encoded, levels 1 .. of a compressed source) count against a 2^28-word limit of their own.
 * The call uploads the given levels. The next plrf_frame records, once and in front of everything else, "textureMipChain.comp" - one execution per level builds
 * that level of every texture that has it, at most 14 whatever the texture count - and "textureBlockEncode.comp", one execution over every block to encode; they
 * run before "sceneMeanAlbedo.comp". The staging buffer is released after that frame. In every other respect the call is plrf_set_scene_textures_formatted: the
 * stores replace one another, texture_count 0 removes, cutoffs and normal maps set afterwards index this store, the same refusals (the bytes of a compressed
 * entry with mip_count 0 are those of level 0), PLR_ERR_UNSUPPORTED on a band / tile pipeline without band_raster, and a refused call changes nothing.
 * plrf_read_scene_texture_store: the words of the texel store as the kernels see it, whichever call made it. *out_word_count receives the count; the words are
 * copied when out_words is not NULL and capacity_words suffices (call once with NULL to size the buffer). PLR_ERR_INVALID_ARGUMENT while there is no store, and
 * before a frame has run since the call that set or built it - the message says so. Waits for the GPU.
 * plrf_get_texture_build_stats: the last build a frame has recorded - executions per pass, texels the chain pass wrote, blocks encoded, bytes of the staging
 * buffer; zeros before there is one. */
typedef struct plrf_scene_texture_source {
    const void* data;
    uint64_t bytes;
    uint32_t width, height, mip_count, format; /* exactly as plrf_scene_texture_data */
    uint32_t store_format;                     /* PLR_FORMAT_RGBA8 | BC1 | BC3 | BC5: what the store is to hold */
} plrf_scene_texture_source;
int plrf_build_scene_textures(void* pipeline, const plrf_scene_texture_source* textures, uint32_t texture_count, const float* const* mesh_uvs, uint32_t mesh_count,
                              const plrf_scene_material* materials, uint32_t draw_count);
int plrf_read_scene_texture_store(void* pipeline, uint32_t* out_words, uint64_t capacity_words, uint64_t* out_word_count);
typedef struct plrf_texture_build_stats {
    uint32_t mip_chain_launches, block_encode_launches; /* executions of "textureMipChain.comp" and of "textureBlockEncode.comp" */
    uint64_t chain_texels, blocks_encoded, staging_bytes;
} plrf_texture_build_stats;
int plrf_get_texture_build_stats(void* pipeline, plrf_texture_build_stats* out);
/* ---- alpha-tested cutouts: depthPrepass.frag:27-30 (sample the albedo texture's alpha with g_mipBias, discard below 0.5) as a per-draw cutoff code 0 .. 255
 * (DESIGN.md "Alpha-tested cutouts in the depth prepass"). 0 is opaque; PLRF_ALPHA_CUTOFF_REFERENCE (128) is the reference's test, a / 255 < 0.5 <=> a <= 127.
 * The alpha code of a fragment is bits 24 - 31 of the albedo word the sampling contract yields for its triangle at that pixel (the draw's constant albedo_rgba8
 * where its material names no albedo texture); a fragment whose alpha code is below its draw's cutoff is no fragment: depth, motion, normal, albedo, specular
 * and everything downstream see what is behind it, or the sky. The counters of plrf_get_prepass_raster_stats do not depend on alpha.
 * plrf_set_scene_alpha_cutoffs needs a scene with textures set; draw_count must be the scene's. The values are copied and take effect with the next frame, in
 * call order. draw_count 0 removes them, and so does every plrf_set_scene_meshes and every plrf_set_scene_textures; they survive
 * plrf_set_scene_mesh_transforms, plrf_set_resolution and plrf_update_settings. While all cutoffs are 0, or none are set, every frame is what it is without this
 * call. PLR_ERR_INVALID_ARGUMENT, with a message that names the cause: no scene set, no textures set, a count mismatch, NULL cutoffs with a non-zero count, a
 * value above 255. PLR_ERR_UNSUPPORTED: a band / tile pipeline without band_raster. A refused call changes nothing. The sun shadow pass has an alpha test of its own, for its own
 * meshes: plrf_set_shadow_caster_cutouts below, and plrf_set_shadow_caster_cutouts_formatted for casters whose cutout textures are BC1 / BC3 / BC5 blocks - both
 * passes take the blocks as they are, and no caller decodes them on the host. */
#define PLRF_ALPHA_CUTOFF_REFERENCE 128u
int plrf_set_scene_alpha_cutoffs(void* pipeline, const uint32_t* cutoffs, uint32_t draw_count);
/* ---- normal maps: triangle.frag:180-196 (shade with normalize(passTBN * normalTexelReconstructed)) as a sixth image of the depth prepass, "shadingNormal" (RGBA8,
 * frame size; DESIGN.md "Normal maps in the depth prepass": the contract in fp64 IEEE operations). normal_textures[d]: PLRF_NO_TEXTURE or an index into the textures
 * given to plrf_set_scene_textures; the texel is the sampling contract's word (same UV, level with g_mipBias, taps, round half even), R and G are x and y.
 * decode PLRF_NORMAL_DECODE_REFERENCE: the reference's reconstruction as written, z = sqrt(1 - x x + 2 y) on the [0, 1] codes, n_t = 2 (x, y, z) - 1;
 * PLRF_NORMAL_DECODE_UNIT: n_t = (2 x - 1, 2 y - 1, sqrt(max(0, 1 - n_t.x^2 - n_t.y^2))). The shading normal is normalize(T n_t.x + B n_t.y + N n_t.z) with the
 * interpolated, not renormalised, per-vertex basis (each vector normalize(mat3(model) v)); where that is zero, and for a draw without a normal texture, it is the
 * vertex normal of the "normal" image. mesh_tangents[k]: 3 floats per vertex of mesh k, NULL (the array or an entry): all (0, 0, 0). mesh_bitangents[k] likewise;
 * NULL (the array or an entry): the host derives normalize(cross(tangent, normal)) per vertex in fp64 (ModelImport.cpp:184), (0, 0, 0) where the length is not a
 * finite number > 0 - which needs a mesh that was given with normals.
 * While normal maps are set the deferred shade reads "shadingNormal" where it read "normal"; the SDF trace and the GI filters keep "normal" (the reference's split:
 * depthPrepass.frag:48 stores the vertex normal). Depth, motion, normal, albedo, specular and the counters never depend on normal maps. The image is created by
 * the first successful call (plrf_get_image(.., "shadingNormal") fails before) and re-created by a resize.
 * plrf_set_scene_normal_maps needs a scene with textures set; mesh_count and draw_count must be the scene's. Everything is copied and takes effect with the next
 * frame, in call order. draw_count 0 removes them, and so does every plrf_set_scene_meshes and every plrf_set_scene_textures; they survive
 * plrf_set_scene_mesh_transforms, plrf_set_scene_alpha_cutoffs, plrf_set_resolution and plrf_update_settings. PLR_ERR_INVALID_ARGUMENT, with a message that names
 * the cause: no scene set, no textures set, a count mismatch, NULL normal_textures with a non-zero count, an index that is neither PLRF_NO_TEXTURE nor <
 * texture_count, a non-finite tangent or bitangent (vertex and mesh are named), a decode other than 1 or 2, NULL bitangents with non-NULL tangents for a mesh
 * given without normals. PLR_ERR_UNSUPPORTED: a band / tile pipeline without band_raster. A refused call changes nothing. */
#define PLRF_NORMAL_DECODE_REFERENCE 1u
#define PLRF_NORMAL_DECODE_UNIT 2u
int plrf_set_scene_normal_maps(void* pipeline, const float* const* mesh_tangents, const float* const* mesh_bitangents, uint32_t mesh_count,
                               const uint32_t* normal_textures, uint32_t draw_count, uint32_t decode);
/* ---- anisotropic filtering of the scene's material textures: the reference samples them through g_sampler_anisotropicRepeat (RenderFrontend.cpp:1305-1314),
 * a sampler with useAnisotropy = true and maxAnisotropy = 8 (ResourceDescriptions.h:169, VulkanSampler.cpp:23). DESIGN.md "Anisotropic filtering in the depth
 * prepass": the contract - per sample N = 1 .. max_anisotropy probes along the major axis of the pixel's footprint, N the smallest integer with N^2 rmin >= rmax,
 * at the mip level of rho2 / N^2, summed in integers and divided by N with round half even; probe count and placement are this contract's (Vulkan leaves them to
 * the implementation). It applies to every sample of the prepass: albedo, specular, the tested alpha of the cutouts and the normal-map texel, RGBA8 and
 * block-compressed alike. max_anisotropy 0 or 1: off, every frame is what it is without this call; 2 .. 16: on (PLRF_ANISOTROPY_REFERENCE, 8: the reference's
 * sampler), from the next recorded frame, in call order. One scalar of pipeline state: it needs neither a scene nor textures (while the scene has none the pass
 * record is what it was) and survives plrf_set_scene_meshes, plrf_set_scene_textures, plrf_set_scene_textures_formatted, plrf_set_scene_alpha_cutoffs,
 * plrf_set_scene_normal_maps, plrf_set_scene_mesh_transforms, plrf_set_resolution and plrf_update_settings. The sun shadow raster's cutout sampling stays
 * isotropic. PLR_ERR_INVALID_ARGUMENT, with a message that names the value: a value above 16. PLR_ERR_UNSUPPORTED: a band / tile pipeline without band_raster. A refused call
 * changes nothing. */
#define PLRF_ANISOTROPY_REFERENCE 8u
int plrf_set_scene_anisotropy(void* pipeline, uint32_t max_anisotropy);
/* ---- alpha-tested cutout casters: sunShadow.frag:17-21 (sample the albedo texture's alpha, discard below 0.5) for the mesh shadow casters (DESIGN.md
 * "Alpha-tested cutout casters in the sun shadow raster"). Casters are another mesh set than the scene's and keep their own copy of the textures:
 * plrf_scene_texture as above (mip_count 0: the host builds the chain), mesh_uvs[k]: 2 floats per vertex of caster mesh k, NULL (the array or an entry): all
 * (0, 0), and one plrf_shadow_cutout per caster draw: the texture whose alpha is tested, or PLRF_NO_TEXTURE (alpha 255 everywhere: the draw stays opaque), and a
 * cutoff code 0 .. 255, 0 = opaque, PLRF_ALPHA_CUTOFF_REFERENCE = the reference's test. A fragment whose alpha code (isotropic trilinear, one level per triangle, no
 * mip bias, UV interpolated with the depth's weights) is below its draw's cutoff casts no shadow; the counters of plrf_get_shadow_raster_stats do not depend on
 * alpha. The pass culls FRONT faces: a single-sided card that faces the light is culled before it is tested, as in the reference - a card that is to cast a
 * shadow from both sides needs both windings.
 * plrf_set_shadow_caster_cutouts needs casters set; mesh_count and draw_count must be the casters'. Everything is copied and takes effect with the next frame, in
 * call order. texture_count 0 removes the cutouts (the other arguments are not looked at), and so does every plrf_set_shadow_casters; they survive
 * plrf_set_shadow_caster_transforms, plrf_set_resolution and plrf_update_settings. While none are set, or all cutoffs are 0, every frame is what it is without
 * this call. PLR_ERR_INVALID_ARGUMENT, with a message that names the cause: no casters set, a count mismatch, a texture size of 0 or above 16384, too many mips
 * for the size, NULL texels, a texture index that is neither PLRF_NO_TEXTURE nor < texture_count, a cutoff above 255, more than 2^28 texels in total, a non-finite
 * UV. PLR_ERR_UNSUPPORTED: a band / tile pipeline without band_raster. A refused call changes nothing. */
typedef struct plrf_shadow_cutout { uint32_t albedo_texture, alpha_cutoff; } plrf_shadow_cutout; /* PLRF_NO_TEXTURE; 0 .. 255, 0 = opaque */
int plrf_set_shadow_caster_cutouts(void* pipeline, const plrf_scene_texture* textures, uint32_t texture_count,
                                   const float* const* mesh_uvs, uint32_t mesh_count,
                                   const plrf_shadow_cutout* cutouts, uint32_t draw_count);
/* ---- block-compressed cutout textures for the casters (DESIGN.md "Block-compressed cutout textures in the sun shadow raster"): plrf_set_shadow_caster_cutouts for
 * textures that carry a format - plrf_scene_texture_data exactly as plrf_set_scene_textures_formatted takes it, so the payload of a DXT5 foliage or fence texture
 * goes in as it is, with neither a host decode nor an RGBA8 copy four times its size. The alpha of a texel is bits 24 - 31 of what the block decode contract yields
 * for it: BC3: its alpha block (both modes); BC1 and BC5: 255, so a draw that names such an entry stays opaque as a draw without a texture does. The pass decodes
 * the alpha block of every BC3 tap in integers and filters the codes as it filters RGBA8 alphas: the maps and counters are exactly those of
 * plrf_set_shadow_caster_cutouts with plr_decode_bc_to_rgba8 of the same levels. Semantics, lifetime and removal are plrf_set_shadow_caster_cutouts': the two
 * calls replace one another's store, texture_count 0 and every plrf_set_shadow_casters remove it, and it survives plrf_set_shadow_caster_transforms,
 * plrf_set_resolution and plrf_update_settings. A call whose entries are all RGBA8 records exactly the pass plrf_set_shadow_caster_cutouts records (an RGBA8 entry
 * with mip_count 0 gets the host's chain). PLR_ERR_INVALID_ARGUMENT, with a message that names the cause: what plrf_set_shadow_caster_cutouts refuses, an unknown
 * format, mip_count 0 on a compressed entry, a bytes mismatch, more than 2^28 words in total (a compressed entry starts at a multiple of 16 bytes).
 * PLR_ERR_UNSUPPORTED: where plrf_set_shadow_caster_cutouts returns it. A refused call changes nothing. */
int plrf_set_shadow_caster_cutouts_formatted(void* pipeline, const plrf_scene_texture_data* textures, uint32_t texture_count,
                                             const float* const* mesh_uvs, uint32_t mesh_count,
                                             const plrf_shadow_cutout* cutouts, uint32_t draw_count);
/* A diagnostic, for tests and tools; a renderer has no use for it. The shape of the "sunShadowRaster.comp" record the last frame with casters made per cascade: *push_bytes is 8 (opaque casters, or all cutoffs 0), 12 (cutouts whose
 * store is all RGBA8, from either call) or 16 (a store with a BC1 / BC3 / BC5 entry: the word textureFormats and binding 14), *storage_buffers the buffers it
 * bound (6, 10 or 11). Zeros before the first frame with casters. Does not wait for the GPU. */
int plrf_get_shadow_raster_record(void* pipeline, uint32_t* push_bytes, uint32_t* storage_buffers);
/* ---- SDF instances of the GI trace from the scene: SDFGI::updateSDFScene (Techniques/SDFGI.cpp:260-313, called from renderScene every frame) as the compute pass
 * "sdfInstanceUpdate.comp", and computeMeanAlbedo (ModelImport.cpp:78-112) as "sceneMeanAlbedo.comp" (DESIGN.md "SDF instances from the scene": the instance
 * contract - padded boxes as plr_sdf_padded_bounds, the world box of the eight transformed corners, worldToLocal = inverse(model translate(bbOffset)) as adjugate
 * over determinant in fp64 rounded once to fp32 - and the mean albedo contract in exact integer sums).
 * plrf_scene_sdf_mesh, one per mesh of the scene: sdf_texture is an index plrf_add_sdf_volume / plrf_add_sdf_volume_dds returned, PLRF_SDF_BAKE (the mesh is baked
 * now, with the asset pipeline's bake at plr_sdf_texture_description's resolution for its local box - the fp32 min / max of its positions -, and registered in the
 * global texture array), or PLRF_NO_TEXTURE (the mesh has no SDF: its draws make no instance, SDFGI.cpp:277-280). The draws whose mesh has an SDF, in draw
 * order, are instances 0 .. n - 1. While a scene SDF is set, every plrf_frame that records the GI trace or the SDF debug view records one execution of
 * "sdfInstanceUpdate.comp" in front of the camera frustum culling: a lane per instance writes sdfInstances ({n, 0, 0, 0}, then n records) and sdfWorldBBs from the
 * model matrices in mainPassMatrices, so an object moved with plrf_set_scene_mesh_transforms takes its occluder and its bounce light with it. "sceneMeanAlbedo.comp"
 * is recorded in front of it in a frame after the texture store or the materials changed (plrf_set_scene_textures*, plrf_set_scene_sdf): an instance's meanAlbedo
 * is the mean of its draw's albedo texture (level 0, the reference's rule: no sRGB decode, the alpha-weighted term truncated per texel; BC5 counts as (R, G, 0,
 * 255)), or the same rule on the draw's constant albedo_rgba8 as a one-texel image (the reference's 0.5 for an untextured mesh is not used: here the constant word
 * is the material), or what plrf_set_scene_sdf_mean_albedo gave for the draw (3 floats per draw; a NaN red = derive; draw_count 0 removes the overrides, and so
 * does every plrf_set_scene_sdf). Without the call nothing is recorded, created or allocated.
 * plrf_set_scene_sdf needs a scene; mesh_count must be the scene's; mesh_count 0 removes the scene SDF, and so does every plrf_set_scene_meshes. It survives
 * plrf_set_scene_mesh_transforms, plrf_set_scene_textures*, plrf_set_resolution and plrf_update_settings. Volumes baked for it are released when it is replaced or
 * removed, and a repeated call re-uses their images: plrf_get_scene_sdf_stats (instances now set, volumes baked and their bytes) does not grow. While it is set,
 * plrf_set_sdf_scene returns PLR_ERR_UNSUPPORTED, and plrf_set_scene_sdf and plrf_set_scene_mesh_transforms refuse a model matrix of an instance whose determinant -
 * the contract's fp64 expression - is zero or not finite; the message names the draw. PLR_ERR_INVALID_ARGUMENT, with a message that names the cause: no scene
 * set, a count mismatch, NULL meshes, an SDF mesh without vertices or with a non-finite position, more instances than max_sdf_instances, a singular matrix, a
 * non-finite override. PLR_ERR_UNSUPPORTED: a band / tile pipeline without band_raster; with band_raster = 1 every rank writes every instance (the SDF scene is
 * not screen-partitioned). A refused call changes nothing. */
#define PLRF_SDF_BAKE 0xfffffffeu
typedef struct plrf_scene_sdf_mesh { uint32_t sdf_texture; } plrf_scene_sdf_mesh;
int plrf_set_scene_sdf(void* pipeline, const plrf_scene_sdf_mesh* meshes, uint32_t mesh_count);
int plrf_set_scene_sdf_mean_albedo(void* pipeline, const float* rgb_or_nan, uint32_t draw_count);
typedef struct plrf_scene_sdf_stats { uint32_t instances, volumes_baked; uint64_t volume_bytes; } plrf_scene_sdf_stats;
int plrf_get_scene_sdf_stats(void* pipeline, plrf_scene_sdf_stats* out);
typedef struct plrf_prepass_raster_stats { uint64_t triangles_submitted, triangles_clipped, subtriangles_drawn, rejects; } plrf_prepass_raster_stats;
int plrf_get_prepass_raster_stats(void* pipeline, plrf_prepass_raster_stats* out);
/* ---- frustum culling of whole draws on the GPU: the bounding-box tests of RenderFrontend::renderScene (RenderFrontend.cpp:565-569 for the camera, :611-646 for
 * the sun) as the compute pass "drawCulling.comp" (DESIGN.md "Frustum culling of draws": the cull contract and the proof). With PLRF_CULL_SCENE every frame
 * that records the depth prepass records one execution in front of it: a lane per draw tests the eight corners of the draw's local box - the fp32 min / max of
 * its mesh's positions, kept by the host from plrf_set_scene_meshes on - under that frame's own jittered mvp against the near plane and the four side planes, with
 * a tolerance of 2^-16 of the box's magnitude (at least 2^-100), and writes a copy of the draw array in which a draw outside one plane has index_count 0. The prepass binds the copy
 * (every wrap strip of a band / tile pipeline too; the test is against the whole frame, never a partition's window). With PLRF_CULL_SHADOW_CASTERS one execution
 * behind lightMatrix.comp does the same for the casters of plrf_set_shadow_casters, per cascade, against the four side planes of that frame's light matrix times
 * the caster's model matrix - the matrices exist only on the GPU when run_light_matrix is 1 -, and each cascade binds its own copy. There is no far plane and no
 * shadow depth plane (the raster contracts decide those per fragment), and a box outside across a frustum edge or corner is kept.
 * Every image the two rasterisers write is byte for byte what it is without culling. While culling is on for a view, plrf_get_prepass_raster_stats and
 * plrf_get_shadow_raster_stats count the kept draws only: submitted, clipped, drawn and rejects are those of the same pass run on the kept draws alone.
 * The flags take effect with the next frame and hold for the pipeline's life until changed, across plrf_set_scene_meshes, plrf_set_shadow_casters,
 * plrf_set_*_transforms, plrf_set_resolution and plrf_update_settings; a flag whose mesh set is absent does nothing until one is set. Flags 0 (the default):
 * nothing is recorded, created or allocated, and every frame is what it is without this call. PLR_ERR_INVALID_ARGUMENT: unknown bits. PLR_ERR_UNSUPPORTED: a
 * band / tile pipeline without band_raster. A refused call changes nothing.
 * plrf_get_draw_culling_stats: the counters of the last frame's cull execution for view 0 (the main pass) or 1 + c (cascade c); waits for the GPU. draws and
 * triangles are the view's totals, visible_* those of the kept draws, culled_by_plane the culled draws by the first plane, in test order, they are outside of.
 * All zero for a view that is off, whose mesh set is absent, or that no frame has rendered yet. A view at or past 1 + sun_shadow_cascade_count is
 * PLR_ERR_INVALID_ARGUMENT. plrf_get_storage_buffer names the outputs once they exist: "sceneCulledDraws" (24 bytes per draw), "sceneCullStats" (8 uint32:
 * visible draws, visible triangles, culled by plane [5], pad), "casterCulledDraws0" .. "casterCulledDraws3" (16 bytes per draw), "casterCullStats" (8 uint32 per
 * cascade). */
#define PLRF_CULL_SCENE          1u   /* the depth prepass's draws, against the frame's own jittered viewProjection */
#define PLRF_CULL_SHADOW_CASTERS 2u   /* the casters, per cascade, against that frame's light matrices */
int plrf_set_draw_culling(void* pipeline, uint32_t flags);
typedef struct plrf_draw_culling_stats {
    uint32_t draws, visible_draws;
    uint64_t triangles, visible_triangles;
    uint32_t culled_by_plane[5];            /* near, +x, -x, +y, -y; shadow views leave [0] at 0 */
} plrf_draw_culling_stats;
int plrf_get_draw_culling_stats(void* pipeline, uint32_t view, plrf_draw_culling_stats* out); /* view 0: main pass; 1 + c: cascade c */
/* ---- debug geometry: the reference's renderDebugGeometry (RenderFrontend.cpp:375-378, 947-956; debug.vert / debug.frag) as the compute pass
 * "debugGeometry.comp" (DESIGN.md "Debug geometry as a compute pass": the line contract in integers, IEEE fp32 and fp64). While flags are set every frame records
 * one execution right behind the deferred shade, in front of skyAndSunSprite.comp and everything else that reads the colour buffer. It draws one-pixel lines into
 * that frame's "color<i>" and "depth<i>", depth-tested GreaterEqual against what the frame wrote, with depth write on as in the reference: a line pixel over the
 * sky gets a depth above 0, so the sky pass leaves it alone, and TAA and the next frame's reprojection see the line's depth. The colour is stored as given, not
 * pre-exposed. PLRF_DEBUG_DRAW_BOXES: the twelve edges of the axis-aligned world box of every scene draw - the eight corners of the mesh's local box under the
 * model matrix of "mainPassMatrices", their fp32 minimum and maximum -, red; with PLRF_CULL_SCENE set only the draws the cull kept. PLRF_DEBUG_SDF_BOXES: the
 * twelve edges of every padded world box the scene SDF (plrf_set_scene_sdf) wrote to "sdfWorldBBs" this frame, green. PLRF_DEBUG_LINES: the caller's segments
 * (camera and cascade frusta, rays, normals). Everything comes from buffers the GPU already holds: no host round trip. A flagged source that is absent - no
 * scene, no scene SDF or a frame without the GI trace, no lines - contributes no segment. Not recorded under sdf_debug_mode, nor on a minimized frame.
 * Flags and lines are copied, take effect with the next recorded frame in call order, and hold across plrf_set_scene_meshes, plrf_set_scene_mesh_transforms,
 * the texture calls, plrf_set_resolution and plrf_update_settings. Flags 0 (the default): nothing is recorded, created or allocated, and every frame is what it
 * is without these calls. PLR_ERR_INVALID_ARGUMENT, with a message that names the cause: an unknown flag bit; null lines with a non-zero count; more than 2^20
 * lines; a non-finite coordinate or colour component, or a negative colour (the line is named). PLR_ERR_UNSUPPORTED: a band / tile pipeline (the pass writes
 * depth and has no halo plan); a pipeline without run_shading. A refused call changes nothing.
 * plrf_get_debug_geometry_stats: the counters of the last frame that recorded the pass; waits for the GPU. submitted: segments the sources held (12 per box,
 * 1 per line); clipped: segments with an end replaced on a clip plane; rejected: segments dropped by a plane or by an end outside the 2^20-pixel band; drawn:
 * segments that reach a pixel column (row, for a steep one) of the image; fragments: fragments that passed the depth test; pixels_written: pixels that changed
 * hands. All zero before the first such frame. plrf_get_storage_buffer names "debugGeometryStats" (8 uint32) and "sceneBounds" (6 floats per draw) once they exist. */
#define PLRF_DEBUG_DRAW_BOXES 1u   /* world AABB of every scene draw: the reference's "Render bounding boxes" */
#define PLRF_DEBUG_SDF_BOXES  2u   /* the padded world boxes of the SDF instances, from "sdfWorldBBs" */
#define PLRF_DEBUG_LINES      4u   /* the caller's segments */
int plrf_set_debug_geometry(void* pipeline, uint32_t flags);          /* 0 = off */
typedef struct plrf_debug_line { float a[3], b[3], rgb[3]; } plrf_debug_line;   /* world space; linear colour, stored as is */
int plrf_set_debug_lines(void* pipeline, const plrf_debug_line* lines, uint32_t count);   /* copied; count 0 removes */
typedef struct plrf_debug_geometry_stats { uint32_t submitted, clipped, rejected, drawn, fragments, pixels_written, pad[2]; } plrf_debug_geometry_stats;
int plrf_get_debug_geometry_stats(void* pipeline, plrf_debug_geometry_stats* out);   /* last frame; waits for the GPU */
/* ---- the frame's noise inputs, generated on the GPU: the four 32 x 32 RG8 void-and-cluster blue-noise textures "noise0" .. "noise3" (generateBlueNoiseTexture,
 * Common/Noise.cpp:232-300, called at RenderFrontend.cpp:1251-1269) as the compute pass "blueNoiseVoidAndCluster.comp", and the 32^3 R8 Perlin volume
 * "perlinNoise3D" of the froxel material pass (generate3DPerlinNoise, Noise.cpp:422-497, Volumetrics.cpp:71-90: 8 grid cells) as "perlinNoise3D.comp" (DESIGN.md
 * "Noise textures as compute passes": the contract in integers and IEEE fp32, and its four deviations from Noise.cpp - rand() is a hash of the seed, the index pitch
 * is the width, the prototype loop stops after N swaps at the latest, the cluster search needs no FLT_MIN start).
 * The next plrf_frame records, once and in front of everything else, four executions of the blue-noise pass (texture t takes streams 2 t and 2 t + 1 of the seed, one
 * 1024-lane block per channel) and / or one of the Perlin pass; the tables the passes read come from plr_noise_gaussian_table and plr_noise_perlin_gradients
 * (plr.h). After that frame the images stay as written until the caller uploads to them or calls again; a call before that frame replaces the seed of the kinds it
 * names. Everything the frame derives from a noise texture (the deferred shade's tap table by noise-texel position) rebuilds itself, as after an upload. Without
 * the call nothing is recorded, created or allocated, and the images hold what the caller uploads (zeros if nothing). The bytes are a pure function of the seed:
 * the ranks of a band / tile partition call it with one seed and agree without an exchange.
 * plrf_get_noise_stats: {swaps, converged, ones, 0} of the prototype loop per texture and channel, as the last blue-noise generation a frame has run wrote them
 * (32 x 32: ones = 102, 28 .. 41 swaps for seeds 1 .. 8); waits for the GPU; zeros before there is one.
 * PLR_ERR_INVALID_ARGUMENT: flags 0 or unknown bits; PLRF_NOISE_PERLIN on a pipeline that has no perlinNoise3D image. A refused call changes nothing. */
#define PLRF_NOISE_BLUE   1u
#define PLRF_NOISE_PERLIN 2u
int plrf_generate_noise(void* pipeline, uint32_t seed, uint32_t flags);
typedef struct plrf_noise_stats { uint32_t status[4][2][4]; } plrf_noise_stats; /* [texture][channel]{swaps, converged, ones, 0} */
int plrf_get_noise_stats(void* pipeline, plrf_noise_stats* out);
/* one iteration of the reference's main loop: record the frame, update camera/UBOs, submit (does not wait for the GPU) */
int plrf_frame(void* pipeline, const plrf_camera* camera, float delta_time, float time);
/* host copies of what the last plrf_frame submitted (340-byte global UBO image, 9 TAA resolve weights) */
int plrf_get_submitted_globals(void* pipeline, void* out_340_bytes);
int plrf_get_resolve_weights(void* pipeline, float* out_9);
int plrf_get_cpu_frame_index(void* pipeline, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif
