"""plrf_raster_window_for (include/plr_frame.h): the tile window a partition's depth prepass is restricted to, as a pure host function - no GPU, no backend.

The expected values are worked out here from the settings alone: the owned rectangle grown, on the sides that have a neighbour, by what the depth downscale
(2 (giHalo + giHistoryHalo) + 16 rows around the band) and the shade with the temporal filter's 3 x 3 dilation behind it (colorHalo + 1) read of the G-buffer
outside the rectangle, must lie inside the window; the window is whole 64 x 64 tiles inside the tile grid; it is the whole grid for an unpartitioned frame and
for whole-image halos; it never shrinks when a halo grows.
"""
import ctypes as C

import pytest

PLRF_HALO_WHOLE_IMAGE = 0xFFFFFFFF
TILE = 64


def _lib():
    from plainrenderer_amd import backend
    lib = backend._load()
    lib.plrf_last_error.restype = C.c_char_p
    return lib


def settings(width, height, rows=None, cols=None, **halos):
    from plainrenderer_amd.frame import PlrfSettings
    s = PlrfSettings()
    assert _lib().plrf_default_settings(C.byref(s), C.c_uint32(width), C.c_uint32(height)) == 0
    if rows:
        s.band_row_begin, s.band_row_end = rows
    if cols:
        s.band_col_begin, s.band_col_end = cols
    for k, v in halos.items():
        setattr(s, k, v)
    return s


def window(s):
    out = (C.c_uint32 * 4)()
    lib = _lib()
    assert lib.plrf_raster_window_for(C.byref(s), out) == 0, lib.plrf_last_error()
    return tuple(int(v) for v in out)


def grid(width, height):
    return (width + TILE - 1) // TILE, (height + TILE - 1) // TILE


def splits(size, parts):
    """`parts` ranges of whole tiles that cover [0, size): the first ones a tile larger where the tiles do not divide"""
    tiles = (size + TILE - 1) // TILE
    bounds = [min(size, TILE * ((tiles * k + parts - 1) // parts)) for k in range(parts)] + [size]
    return list(zip(bounds[:-1], bounds[1:]))


def partitions(width, height, nx, ny):
    """[(rows, cols or None)] of an nx x ny partition; nx == 1: bands"""
    return [(rows, cols if nx > 1 else None) for rows in splits(height, ny) for cols in splits(width, nx)]


def needed(s, width, height, rows, cols):
    """the pixel rectangle [x0, x1) x [y0, y1) the window must contain: the owned one grown by the two reaches on the sides with a neighbour"""
    cap = max(width, height)
    gi = 0 if s.band_gi_halo == 0xFFFFFFFE else min(s.band_gi_halo, cap)
    reach = max(2 * (gi + min(s.band_gi_history_halo, cap)) + 16, s.band_color_halo + 1)

    def grow(begin, end, size):
        return (max(begin - reach, 0) if begin > 0 else 0), (min(end + reach, size) if end < size else size)
    y0, y1 = grow(rows[0], rows[1], height)
    x0, x1 = grow(cols[0], cols[1], width) if cols else (0, width)
    return x0, y0, x1, y1


FRAMES = ((1920, 1080), (1000, 700), (3840, 2160))
SHAPES = ((1, 2), (1, 3), (2, 2), (4, 3))  # (nx, ny): 2 and 3 bands, 2 x 2 and 4 x 3 tiles
SMALL = dict(band_gi_halo=8, band_gi_history_halo=4)
WHOLE = dict(band_gi_halo=PLRF_HALO_WHOLE_IMAGE)


def test_default_settings_leave_band_raster_off_and_the_struct_sizes_agree():
    from plainrenderer_amd.frame import PlrfSettings
    size = C.sizeof(PlrfSettings)
    buf = (C.c_uint8 * (size + 64))(*([0xA5] * (size + 64)))
    assert _lib().plrf_default_settings(buf, C.c_uint32(640), C.c_uint32(360)) == 0
    s = PlrfSettings.from_buffer_copy(bytes(buf)[:size])
    assert s.band_raster == 0 and (s.width, s.height) == (640, 360)
    assert PlrfSettings.band_raster.offset + 8 == size and PlrfSettings.run_sky.offset + 4 == size, "band_raster stands with the band fields, in front of run_sky, the last field"
    assert all(b == 0xA5 for b in bytes(buf)[size:]), "the C struct is larger than the ctypes mirror"
    assert bytes(buf)[size - 4:size] == bytes(4), "the C struct is smaller than the ctypes mirror: its last field was not written"


@pytest.mark.parametrize("width,height", FRAMES)
def test_an_unpartitioned_frame_has_the_whole_grid(width, height):
    for halos in ({}, SMALL, WHOLE, dict(band_raster=1)):
        assert window(settings(width, height, **halos)) == (0, 0) + grid(width, height)


@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("width,height", FRAMES)
def test_whole_image_halos_have_the_whole_grid(width, height, nx, ny):
    for rows, cols in partitions(width, height, nx, ny):
        assert window(settings(width, height, rows, cols, **WHOLE)) == (0, 0) + grid(width, height)


@pytest.mark.parametrize("halos", [SMALL, {}, dict(band_gi_halo=0xFFFFFFFE), dict(SMALL, band_color_halo=100)], ids=["small", "default", "requested", "wide_colour"])
@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("width,height", FRAMES)
def test_the_window_is_tile_aligned_inside_the_grid_and_contains_what_the_passes_read(width, height, nx, ny, halos):
    gx, gy = grid(width, height)
    for rows, cols in partitions(width, height, nx, ny):
        s = settings(width, height, rows, cols, **halos)
        x0, y0, x1, y1 = window(s)
        assert 0 <= x0 < x1 <= gx and 0 <= y0 < y1 <= gy, "half-open, not empty, inside the %d x %d grid: %r" % (gx, gy, (x0, y0, x1, y1))
        nx0, ny0, nx1, ny1 = needed(s, width, height, rows, cols)
        assert x0 * TILE <= nx0 and y0 * TILE <= ny0 and min(x1 * TILE, width) >= nx1 and min(y1 * TILE, height) >= ny1, \
            "rows %r cols %r: the window %r does not contain %r" % (rows, cols, (x0, y0, x1, y1), (nx0, ny0, nx1, ny1))
        # no growth on a side without a neighbour, and none past the frame: a band's window spans every tile column
        if cols is None:
            assert (x0, x1) == (0, gx)
        if rows[0] == 0:
            assert y0 == 0
        if rows[1] == height:
            assert y1 == gy
        assert window(settings(width, height, rows, cols, band_raster=1, **halos)) == (x0, y0, x1, y1), "the window does not depend on band_raster"


def test_small_halos_leave_tiles_out():
    """the point of the window: with small halos a 4K quadrant's window is not the frame (the reach is 2 (8 + 4) + 16 + 1 = 41 pixels: one more tile per inner side)"""
    (rows, cols) = partitions(3840, 2160, 2, 2)[0]
    assert (rows, cols) == ((0, 1088), (0, 1920))
    assert window(settings(3840, 2160, rows, cols, **SMALL)) == (0, 0, 31, 18)
    rows, _ = partitions(3840, 2160, 1, 4)[1]
    assert rows == (576, 1088)
    assert window(settings(3840, 2160, rows, None, **SMALL)) == (0, 8, 60, 18)


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_the_window_is_monotone_in_every_halo(nx, ny):
    width, height = 1920, 1080
    steps = dict(band_gi_halo=(0, 1, 8, 31, 64, 500, 5000, PLRF_HALO_WHOLE_IMAGE), band_gi_history_halo=(0, 4, 16, 100, 1000, 100000),
                 band_color_halo=(0, 8, 63, 64, 200, 3000), band_post_halo=(0, 224, 1000), band_taa_history_halo=(0, 32, 1000))
    for rows, cols in partitions(width, height, nx, ny):
        for field, values in steps.items():
            previous = None
            for v in values:
                x0, y0, x1, y1 = window(settings(width, height, rows, cols, **dict(SMALL, **{field: v})))
                if previous:
                    assert x0 <= previous[0] and y0 <= previous[1] and x1 >= previous[2] and y1 >= previous[3], "%s = %d shrinks the window of rows %r cols %r" % (field, v, rows, cols)
                previous = (x0, y0, x1, y1)


def wrap_strips(s):
    out, count = (C.c_uint32 * 12)(), C.c_uint32()
    assert _lib().plrf_raster_wrap_strips_for(C.byref(s), out, C.byref(count)) == 0
    return [tuple(int(v) for v in out[4 * k:4 * k + 4]) for k in range(count.value)]


@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("width,height", FRAMES)
def test_wrap_strips_lie_at_the_opposite_frame_edge(width, height, nx, ny):
    """the temporal GI filter's repeat-addressed read of last frame's motion: a window that touches a frame edge without spanning the frame in that direction gets
    the opposite edge's tile column over its rows, the opposite edge's tile row over its columns, and the opposite corner; none with whole-image halos"""
    gx, gy = grid(width, height)
    for rows, cols in partitions(width, height, nx, ny):
        assert wrap_strips(settings(width, height, rows, cols, **WHOLE)) == []
        s = settings(width, height, rows, cols, **SMALL)
        x0, y0, x1, y1 = window(s)
        far_x = None if (x0 == 0 and x1 == gx) else gx - 1 if x0 == 0 else 0 if x1 == gx else None
        far_y = None if (y0 == 0 and y1 == gy) else gy - 1 if y0 == 0 else 0 if y1 == gy else None
        expected = ([(far_x, y0, far_x + 1, y1)] if far_x is not None else []) + ([(x0, far_y, x1, far_y + 1)] if far_y is not None else [])
        if far_x is not None and far_y is not None:
            expected.append((far_x, far_y, far_x + 1, far_y + 1))
        assert wrap_strips(s) == expected, "rows %r cols %r window %r" % (rows, cols, (x0, y0, x1, y1))
    assert wrap_strips(settings(width, height)) == [], "an unpartitioned frame has none"


def test_null_arguments_are_refused():
    lib = _lib()
    out = (C.c_uint32 * 4)()
    assert lib.plrf_raster_window_for(None, out) == -1 and lib.plrf_raster_window_for(C.byref(settings(64, 64)), None) == -1
    assert lib.plrf_get_raster_window(None, out) == -1
