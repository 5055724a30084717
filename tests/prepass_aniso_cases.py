"""Inputs of the anisotropic filtering tests of "depthPrepassRaster.comp" (tests/test_prepass_aniso.py, tests/test_prepass_aniso_cpu.py): named cases at the smallest
shapes at which the probe loop can still go wrong, each with a check, on the reference alone, that the case is what it is for.

A run is (prepass case, texture store, normal inputs or None, cutoffs or None, A): the dict of tests/prepass_raster_cases.py, a store of
tests/prepass_texture_cases.py (all RGBA8) or tests/prepass_bc_cases.py (mixed, with `formats`), what tests/prepass_normal_cases.py and
tests/prepass_alpha_cases.py hand their references, and the execution's maxAnisotropy. Frames are 64 x 48 or 70 x 66 (one is 64 x 64, see face_on), textures at
most 64 x 64 with full chains.
  floor          a ground quad from behind the camera to the distance, a 64 x 64 random-texel RGBA8 chain, A = 8: every N from 2 to 8 on the floor (N = 1 needs
                 rmin == rmax exactly, which no perspective pixel has: a post with the constant UV (0, 0), rmax = 0, stands on the floor for it), and L0 below the
                 isotropic contract's
  major_x, major_y   affine quads with ax = (3, 1 / 4), ay = (1 / 2, 1) texels and the same with the axes exchanged: rx > ry throughout in one, ry > rx in the other
  odd_counts     the floor with A = 5 and A = 16: N = 3, 5, 6, 7 occur; and an affine quad with N = 3 and N = 2 whose probes hit texel centres along u at level 0
                 (fw = 0): channels that land exactly on a half, 2 rem == D, with both parities of qd
  degenerate     a quad whose u depends on x alone and whose v is constant (rmin = 0: N = A) beside one with the constant UV (0, 0) (rmax = 0: N = 1)
  wrap           probes across the repeat seam and at negative UVs; and UVs that reach 2^20 in the last column: the centre is valid, the probes beyond it are not
  face_on        a magnified quad with A = 16 on a 64 x 64 frame - with both sizes a power of two every operation of the footprint is exact, so rx == ry exactly and
                 N = 1 everywhere; at 64 x 48 rounding leaves rmin < rmax by an ulp on most pixels, which is N = 2 - and the result is the isotropic pass'
  bc_alpha       a BC3 albedo whose alpha makes holes, under cutoff 128 on the floor, A = 8
  bc5_normal     a BC5 normal map on the floor under both decodes, A = 8
  mixed_ragged   70 x 66, two floor halves over a store that mixes RGBA8, BC1, BC3 and BC5, g_mipBias -0.75 and +1.5, A = 8
"""
import numpy as np

import prepass_alpha_cases as ac
import prepass_aniso_reference as aniso
import prepass_bc_cases as bc
import prepass_normal_cases as nc
import prepass_normal_reference as nref
import prepass_raster_cases as pc
import prepass_raster_reference as ref
import prepass_texture_cases as tc
import prepass_texture_reference as tref
from shadow_raster_cases import quad

F32 = np.float32
NONE = tref.NONE
RGBA8, BC1, BC3, BC5 = bc.RGBA8, bc.BC1, bc.BC3, bc.BC5
UV_SCALE = 1.5  # world units per UV unit on the floor
FORWARD = (0.0, 0.36, 1.0)  # pitched 20 degrees towards the floor (y = +1.5): the view meets it at 37 degrees in the first rows and at 3 in the last


def random_chain(size, seed):
    """a size x size RGBA8 texture of random texels with the full chain"""
    level0 = np.random.default_rng(seed).integers(0, 1 << 32, size * size, dtype=np.uint64).astype(np.uint32)
    return tc.chain(level0, size, size), size, size, tref.full_mip_count(size, size)


def floor_case(width, height, strips=((-40.0, 40.0),), post=False, y=1.5):
    """ground quads (one draw per x range, both windings: one faces the camera) under a camera at the origin looking down +z; UV = (x, z) / UV_SCALE.
    post: one more draw, a quad standing on the floor with the UV (0, 0) at all its vertices"""
    cam = pc.camera(forward=FORWARD, aspect=width / height, near=0.1, far=300.0)
    vp = np.asarray(cam.view_projection(), F32).reshape(16)
    positions, indices, draws = [], [], []
    for x0, x1 in strips:
        base = 4 * len(draws)
        positions += [[x0, y, -5.0], [x1, y, -5.0], [x1, y, 200.0], [x0, y, 200.0]]
        indices += [base + k for k in (0, 2, 1, 0, 3, 2, 0, 1, 2, 0, 2, 3)]
        draws.append([12 * len(draws), 12, 0, 0])
    positions = np.asarray(positions, F32)
    uvs = np.stack([positions[:, 0] / F32(UV_SCALE), positions[:, 2] / F32(UV_SCALE)], axis=1).astype(F32)
    if post:
        base = positions.shape[0]
        positions = np.concatenate([positions, np.asarray([[-0.4, y, 6.0], [0.4, y, 6.0], [0.4, y - 1.2, 6.0], [-0.4, y - 1.2, 6.0]], F32)])
        uvs = np.concatenate([uvs, np.zeros((4, 2), F32)])
        indices += [base + k for k in (0, 2, 1, 0, 3, 2, 0, 1, 2, 0, 2, 3)]
        draws.append([12 * len(draws), 12, 0, 0])
    return pc.make_case(width, height, ref.main_pass_matrices(vp, vp, [pc.IDENTITY]), positions, indices, draws), uvs


def _floor(A=8, seed=1):
    case, uvs = floor_case(64, 48, post=True)
    return tc.textured(case, uvs, [(0, 0), (0, 0)], [random_chain(64, seed)]) + (None, None, A)


def _major(exchanged):
    case = pc.pixel_case([quad(0.0, 0.0, 64.0, 48.0, 0.5, 0.5)], 64, 48)
    fn = (lambda x, y: ((0.5 * x + 3.0 * y) / 64.0, (x + 0.25 * y) / 64.0)) if exchanged else (lambda x, y: ((3.0 * x + 0.5 * y) / 64.0, (0.25 * x + y) / 64.0))
    return [tc.textured(case, tc.pixel_uvs(case, fn), [(0, 1)], [random_chain(64, 2), random_chain(32, 3)]) + (None, None, 8)]


def _ties():
    """left: u = 3 x / 64, v = 17 / 16 y / 64 on the 64 x 64 texture - ax = (3, 0), ay = (0, 17 / 16), N = 3 (4 ry < rx <= 9 ry with room on both sides), the probes
    of a pixel at the texel centres 3 i, 3 i + 1, 3 i + 2 (fx = 0) and fy a multiple of 8; right: 2 texels per pixel, N = 2. r = rx / N^2 = 1: lod 0, fw = 0. T is
    then a multiple of 2^19 and lands on a half of D = N 2^24 once in 32 N"""
    case = pc.pixel_case([quad(0.0, 0.0, 32.0, 48.0, 0.5, 0.5), quad(32.0, 0.0, 64.0, 48.0, 0.5, 0.5)], 64, 48)
    uvs = tc.quad_uvs(case, [lambda x, y: (3.0 * x / 64.0, 1.0625 * y / 64.0), lambda x, y: (2.0 * x / 64.0, 1.0625 * y / 64.0)])
    return tc.textured(case, uvs, [(0, 0), (0, 0)], [random_chain(64, 4)]) + (None, None, 16)


def _odd_counts():
    return [_floor(5), _floor(16), _ties()]


def _degenerate():
    case = pc.pixel_case([quad(0.0, 0.0, 32.0, 48.0, 0.5, 0.5), quad(32.0, 0.0, 64.0, 48.0, 0.5, 0.5)], 64, 48)
    uvs = tc.quad_uvs(case, [lambda x, y: (2.0 * x / 64.0, 0.375 + 0.0 * y), lambda x, y: (0.0 * x, 0.0 * y)])
    return [tc.textured(case, uvs, [(0, 0), (0, 0)], [random_chain(64, 5)]) + (None, None, A) for A in (8, 5)]


LIMIT_LEFT, LIMIT_RIGHT = 1048576.0 - 15.9375, 1048576.0 + 0.125  # float32 values; the last column's centre lies 2^-11 below 2^20


def _wrap():
    """top: u from -2 to 2 (4 texels per pixel) and v from -0.05 to 0.04375 (1 / 4 texel per pixel): seams at u = -1, 0, 1 and at v = 0, negative UVs. bottom: u from
    2^20 - 15.9375 to 2^20 + 0.125 over 64 pixels - about 16 texels per pixel, N = 8 - and v at 1 texel per pixel"""
    case = pc.pixel_case([quad(0.0, 0.0, 64.0, 24.0, 0.5, 0.5), quad(0.0, 24.0, 64.0, 48.0, 0.5, 0.5)], 64, 48)
    uvs = tc.quad_uvs(case, [lambda x, y: (-2.0 + 4.0 * x / 64.0, -0.05 + 0.09375 * y / 24.0), lambda x, y: (LIMIT_LEFT + (LIMIT_RIGHT - LIMIT_LEFT) * x / 64.0, (y - 24.0) / 64.0)])
    assert float(uvs[:, 0].max()) == LIMIT_RIGHT and float(np.sort(np.unique(uvs[:, 0]))[-2]) == LIMIT_LEFT
    return [tc.textured(case, uvs, [(0, 0), (0, 0)], [random_chain(64, 6)]) + (None, None, 8)]


def _face_on():
    case = pc.pixel_case([quad(0.0, 0.0, 64.0, 64.0, 0.5, 0.5)], 64, 64)
    uvs = tc.pixel_uvs(case, lambda x, y: (x / 256.0, y / 256.0))
    return [tc.textured(case, uvs, [(0, 1)], [random_chain(64, 7), random_chain(16, 8)]) + (None, None, 16)]


def _bc_alpha():
    case, uvs = floor_case(64, 48)
    tex = bc.store(case, uvs, [(0, NONE)], [bc.full(BC3, 64, 64, 9, alpha_binary=True)])
    return [(case, tex, None, np.array([ac.REFERENCE_CUTOFF], np.uint32), 8)]


def _bc5_normal():
    runs = []
    for decode in (nref.DECODE_REFERENCE, nref.DECODE_UNIT):
        case, uvs = floor_case(64, 48)
        case = nc.with_normals(case, (0.0, -1.0, 0.0))
        tex = bc.store(case, uvs, [(1, NONE)], [bc.full(BC5, 64, 64, 10), bc.full(BC1, 32, 32, 11)])
        runs.append((case, tex, nc.normal_inputs(case, (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), [0], decode), None, 8))
    return runs


def _mixed_ragged():
    runs = []
    for mip_bias in (-0.75, 1.5):
        case, uvs = floor_case(70, 66, strips=((-40.0, 0.0), (0.0, 40.0)))
        rgba = random_chain(32, 12) + (RGBA8,)
        runs.append((case, bc.store(case, uvs, [(0, 1), (2, 3)], [rgba, bc.full(BC1, 64, 64, 13), bc.full(BC3, 64, 32, 14), bc.full(BC5, 32, 64, 15)], mip_bias=mip_bias), None, None, 8))
    return runs


CASES = dict(floor=lambda: [_floor()], major_x=lambda: _major(False), major_y=lambda: _major(True), odd_counts=_odd_counts, degenerate=_degenerate, wrap=_wrap,
             face_on=_face_on, bc_alpha=_bc_alpha, bc5_normal=_bc5_normal, mixed_ragged=_mixed_ragged)

_reference_cache = {}


def compute(case, tex, nm, cutoffs, A, diagnostics=True):
    """-> (the five images, keys, counters and diagnostics; shadingNormal or None; its diagnostics or None)"""
    base = aniso.base_images(case, tex, cutoffs, A, diagnostics=diagnostics)
    details = {}
    sn = None if nm is None else aniso.shade(case, tex, nm, base["keys"], base["normal"], A, details=details)
    return base, sn, (details if nm is not None else None)


def reference(name):
    """[(case, store, normal inputs, cutoffs, A, base, shadingNormal or None, its diagnostics or None)], computed once; callers must not modify it"""
    if name not in _reference_cache:
        _reference_cache[name] = [run + compute(*run) for run in CASES[name]()]
    return _reference_cache[name]


def isotropic(run):
    """the same run under the isotropic contract, by the existing references: (base, shadingNormal or None)"""
    case, tex, nm, cutoffs = run[:4]
    decoded = aniso._decoded(tex)
    base = nc.base_images(case, decoded, cutoffs)
    return base, (None if nm is None else nref.shade(case, decoded, nm, base["keys"], base["normal"]))


def _draw_of(case, base):
    import prepass_alpha_reference as aref
    return aref.winner_draw(case, base["keys"])


def _check_floor(runs):
    (case, tex, nm, cutoffs, A, base, sn, _), = runs
    d = base["diagnostics"]["albedo"]
    draw = _draw_of(case, base)
    assert sorted(np.unique(d["N"][draw == 0]).tolist()) == list(range(2, 9)), "every N from 2 to 8 on the floor: %r" % np.unique(d["N"][draw == 0]).tolist()
    assert (draw == 1).sum() > 20 and (d["N"][draw == 1] == 1).all(), "the post: rmax = 0, N = 1"
    iso = tref.sample(case, tex, base["keys"], diagnostics=True)["diagnostics"]["albedo"]
    lower = (d["L0"] < iso["L0"]) & (draw == 0)
    assert lower.sum() > 200 and not (d["L0"] > iso["L0"]).any(), "the level is lower than the isotropic contract's on %d pixels" % lower.sum()
    assert (d["fell"][draw >= 0] == 0).all()
    assert not np.array_equal(base["albedo"], isotropic(runs[0])[0]["albedo"])


def _check_major(runs, major_x):
    (case, tex, nm, cutoffs, A, base, sn, _), = runs
    for name in ("albedo", "specular"):
        d = base["diagnostics"][name]
        assert (base["keys"] != 0).all() and (d["major_x"] == (1 if major_x else 0)).all() and (d["N"] == 3).all(), "rmax / rmin = 9.0625 / 1.25: N = 3"
    assert not np.array_equal(base["albedo"], isotropic(runs[0])[0]["albedo"])


def _check_odd_counts(runs):
    assert [run[4] for run in runs] == [5, 16, 16]
    seen = [set(np.unique(run[5]["diagnostics"]["albedo"]["N"]).tolist()) for run in runs]
    assert {3, 5} <= seen[0] and max(seen[0]) == 5 and {3, 5, 6, 7} <= seen[1] and max(seen[1]) == 16, "N on the floor: %r, %r" % (seen[0], seen[1])
    case, tex, nm, cutoffs, A, base, sn, _ = runs[2]
    d = base["diagnostics"]["albedo"]
    assert (d["N"][:, :32] == 3).all() and (d["N"][:, 32:] == 2).all() and (d["L0"] == 0).all() and (d["fw"] == 0).all()
    ties = np.asarray(d["ties"])
    assert (ties & 1 == 0).sum() > 10 and (ties & 1 == 1).sum() > 10, "channels exactly on a half with qd even and qd odd: %d, %d" % ((ties & 1 == 0).sum(), (ties & 1 == 1).sum())
    # the ties of the N = 3 half alone: the division by a D that is no power of two decides them
    left = aniso.sample(case, tex, np.where(np.arange(64)[None, :] < 32, base["keys"], np.uint64(0)), A, diagnostics=True)["diagnostics"]["albedo"]["ties"]
    left = np.asarray(left)
    assert (left & 1 == 0).sum() > 3 and (left & 1 == 1).sum() > 3, "N = 3: %d even, %d odd" % ((left & 1 == 0).sum(), (left & 1 == 1).sum())


def _check_degenerate(runs):
    for case, tex, nm, cutoffs, A, base, sn, _ in runs:
        d = base["diagnostics"]["albedo"]
        assert (d["N"][:, :32] == A).all(), "v constant: rmin = 0, N = A"
        assert (d["N"][:, 32:] == 1).all(), "the constant UV (0, 0): rmax = 0, N = 1"
        assert np.unique(base["albedo"][:, 32:]).size == 1 and np.unique(base["albedo"][:, :32]).size == 32, "one word on the right; on the left one per column, v being constant"


def _check_wrap(runs):
    (case, tex, nm, cutoffs, A, base, sn, _), = runs
    d = base["diagnostics"]["albedo"]
    assert (d["N"] == 8).all()
    assert (d["fell"][:24] == 0).all()
    assert (d["fell"][24:, 63] == 1).all() and (d["fell"][24:, :63] == 0).all(), "the last column of the lower quad: probes at or beyond 2^20"
    # the centre of that column is valid: the isotropic contract samples there, and not at (0, 0)
    u = LIMIT_LEFT + (LIMIT_RIGHT - LIMIT_LEFT) * 63.5 / 64.0
    assert u < 1048576.0 and u + (7.0 / 16.0) * (LIMIT_RIGHT - LIMIT_LEFT) / 64.0 >= 1048576.0
    assert not np.array_equal(base["albedo"], isotropic(runs[0])[0]["albedo"])


def _check_face_on(runs):
    (case, tex, nm, cutoffs, A, base, sn, _), = runs
    assert A == 16 and (case["width"], case["height"]) == (64, 64)
    for name in ("albedo", "specular"):
        assert (base["diagnostics"][name]["N"] == 1).all() and (base["diagnostics"][name]["L0"] == 0).all()
    iso = isotropic(runs[0])[0]
    assert np.array_equal(base["albedo"], iso["albedo"]) and np.array_equal(base["specular"], iso["specular"])


def _check_bc_alpha(runs):
    (case, tex, nm, cutoffs, A, base, sn, _), = runs
    assert int(tex["formats"][0]) == BC3
    iso = isotropic(runs[0])[0]
    holes, iso_holes = base["keys"] == 0, iso["keys"] == 0
    covered = pc.rasterise(case)["keys"] != 0
    assert 100 < (holes & covered).sum() < covered.sum() - 100, "the floor has holes and is not all holes"
    assert ((holes != iso_holes) & covered).sum() > 20, "the hole set differs from the isotropic run's"
    assert ((base["albedo"][~holes] >> np.uint32(24)) >= 128).all()
    assert not np.array_equal(base["depth"], iso["depth"])


def _check_bc5_normal(runs):
    assert [run[2]["decode"] for run in runs] == [nref.DECODE_REFERENCE, nref.DECODE_UNIT]
    for run in runs:
        case, tex, nm, cutoffs, A, base, sn, details = run
        won = base["keys"] != 0
        assert int(tex["formats"][0]) == BC5 and won.sum() > 1000
        assert (details["N"][won] >= 2).all() and np.unique(details["N"][won]).size >= 5
        assert np.unique(sn[won]).size > 100 and not np.array_equal(sn, base["normal"]) and not (sn[~won]).any()
        assert not np.array_equal(sn, isotropic(run)[1])
    assert not np.array_equal(runs[0][6], runs[1][6]), "the decodes differ"


def _check_mixed_ragged(runs):
    assert [run[1]["mip_bias"] for run in runs] == [-0.75, 1.5]
    for case, tex, nm, cutoffs, A, base, sn, _ in runs:
        assert (case["width"], case["height"]) == (70, 66) and tex["formats"].tolist() == [RGBA8, BC1, BC3, BC5]
        draw = _draw_of(case, base)
        for name in ("albedo", "specular"):
            for k in (0, 1):
                assert np.unique(base[name][draw == k]).size > 100 and np.unique(base["diagnostics"][name]["N"][draw == k]).size >= 5
    assert (runs[0][5]["diagnostics"]["albedo"]["L0"] < runs[1][5]["diagnostics"]["albedo"]["L0"]).any()


CASE_CHECKS = dict(floor=_check_floor, major_x=lambda runs: _check_major(runs, True), major_y=lambda runs: _check_major(runs, False), odd_counts=_check_odd_counts,
                   degenerate=_check_degenerate, wrap=_check_wrap, face_on=_check_face_on, bc_alpha=_check_bc_alpha, bc5_normal=_check_bc5_normal,
                   mixed_ragged=_check_mixed_ragged)


def check_case_is_what_it_is_for(name):
    CASE_CHECKS[name](reference(name))
