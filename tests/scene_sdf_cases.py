"""Inputs of the scene SDF tests (tests/test_scene_sdf_cpu.py, tests/test_scene_sdf.py, tests/test_scene_sdf_frame.py): the smallest shapes at which
"sdfInstanceUpdate.comp" and "sceneMeanAlbedo.comp" can still go wrong.

Instance cases: 1, 63, 64, 65 and 257 instances (one lane, the edges of a wave, more than one block of 64), `alternate` (ten draws, every second one's mesh
has no SDF: the instance map is not the identity) and `empty` (no instance: the header alone). Instance i of a count case takes matrix i mod 9 and box
(i // 9) mod 3, so from 27 instances on every matrix meets every box. The matrices: identity, a translation, a rotation about a skew axis, a non-uniform scale
with a negative factor, scales of 1e-3 and 1e3, a shear, a matrix whose last row is not (0, 0, 0, 1), and one whose inverse leaves fp32 in an element (x scaled by
2^-100 and translated by 2^100: the inverse's translation is -2^200) while its fp64 determinant is 2^-100. The boxes: a 2 m cube, a 9 x 1 x 3 m slab (0.075 of the
extent exceeds the 0.5 minimum on x alone), a quad with no extent in y. The mean albedo of a draw comes, by draw index mod 3, from an override, from the mean
albedo buffer (arbitrary values: the instance pass only copies them) or from the draw's constant word, whose alpha runs through 0, 1, 127, 128 and 255.
Both output buffers are prefilled with a pattern and hold three instances more than the case writes.

The mean albedo store: RGBA8 1 x 1, 3 x 5, 64 x 64, 260 x 4 (alphas 0, 1, 127, 128, 255 and random; the odd sizes in front
put them at addresses that are no multiple of 16), 7 x 9 all 255, 512 x 512 random with alphas from 128 up (its sums need more than 24
bits: the conversion to fp32 rounds), one texture no draw names (its slot keeps the sentinel), BC1 with punch-through blocks and BC3 at one block and at 8 x 12,
BC3 at 5 x 7 (a level 0 that is no multiple of 4: its blocks reach past the level) and BC5 at 8 x 8. Two draws share the 3 x 5 texture, one draw names none, one
names an index beyond the store.
"""
import struct

import numpy as np

import prepass_bc_cases as bc
import prepass_bc_reference as bref
import scene_sdf_reference as ref

F32, U32 = np.float32, np.uint32
NONE = ref.NONE
COUNTS = (1, 63, 64, 65, 257)
EXTRA = 3  # instances of room behind the last one written
SENTINEL = F32(-7.25)


def _mat(rows):
    """4 x 4 in mathematical row / column order -> 16 floats, glm column-major"""
    return np.asarray(rows, np.float64).T.reshape(16).astype(F32)


def _rotation(axis, angle):
    x, y, z = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    c, s = np.cos(angle), np.sin(angle)
    r = np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s], [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
                  [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)]])
    m = np.eye(4)
    m[:3, :3] = r
    m[:3, 3] = (0.5, -2.0, 7.25)
    return _mat(m)


MATRICES = dict(
    identity=_mat(np.eye(4)),
    translation=_mat([[1, 0, 0, 3.5], [0, 1, 0, -0.25], [0, 0, 1, 12.0], [0, 0, 0, 1]]),
    rotation=_rotation((1.0, 2.0, -0.5), 0.7),
    mirror=_mat([[-1.5, 0, 0, 1], [0, 0.75, 0, 2], [0, 0, 2.25, 3], [0, 0, 0, 1]]),
    small=_mat([[1e-3, 0, 0, 1], [0, 1e-3, 0, 1], [0, 0, 1e-3, 1], [0, 0, 0, 1]]),
    large=_mat([[1e3, 0, 0, -40], [0, 1e3, 0, 8], [0, 0, 1e3, 0.5], [0, 0, 0, 1]]),
    shear=_mat([[1, 0.5, -0.25, 0], [0, 1, 0.75, 1], [0, 0, 1, -2], [0, 0, 0, 1]]),
    projective=_mat([[1, 0, 0.5, 2], [0, 1.25, 0, -1], [0.25, 0, 1, 0], [0.25, 0, 0.125, 2]]),
    overflow=_mat([[2.0 ** -100, 0, 0, 2.0 ** 100], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]),
)
MATRIX_NAMES = tuple(MATRICES)
BOXES = dict(cube=((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), slab=((-4.5, -0.5, -1.5), (4.5, 0.5, 1.5)), quad=((-2.0, 0.75, -1.0), (1.0, 0.75, 3.0)))
BOX_NAMES = tuple(BOXES)
ALPHAS = (0, 1, 127, 128, 255)


def _pattern_bytes(n, salt):
    return ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt)) >> np.uint64(7)).astype(np.uint8).tobytes()


def _box(name):
    mn, mx = BOXES[name]
    return np.asarray(mn, F32), np.asarray(mx, F32)


def instance_case(name):
    """the inputs of one execution of "sdfInstanceUpdate.comp" (scene_sdf_reference.instance_pass takes the same dict)"""
    if name == "empty":
        draws, instance_draws = 2, []
    elif name == "alternate":
        draws, instance_draws = 10, [0, 2, 4, 6, 8]
    else:
        draws = int(name)
        instance_draws = list(range(draws))
    models = np.stack([MATRICES[MATRIX_NAMES[d % 9]] for d in range(draws)])
    table = [(d, 5 + 3 * d, *_box(BOX_NAMES[(d // 9) % 3])) for d in instance_draws]
    rng = np.random.default_rng(0x5DF + draws)
    words = [int(rng.integers(0, 1 << 24)) | (ALPHAS[d % 5] << 24) for d in range(draws)]
    overrides = np.full((draws, 3), np.nan, F32)
    overrides[0::3] = rng.uniform(0.0, 1.0, (len(range(0, draws, 3)), 3)).astype(F32)
    textures = 4
    materials = np.full((draws, 2), NONE, U32)
    materials[1::3, 0] = np.arange(len(range(1, draws, 3))) % textures  # (draws 0 mod 3 have an override, which wins; draws 2 mod 3 have the constant word)
    materials[0::3, 0] = 1
    means = rng.uniform(0.0, 1.0, (textures, 4)).astype(F32)
    n = len(table)
    # MainPassMatrices: model, then mvp and mvpPrevious, which the pass does not read
    matrices = np.concatenate([models, rng.normal(size=(draws, 32)).astype(F32)], axis=1)
    draw_records = np.zeros((draws, 6), U32)
    draw_records[:, 4] = words
    return dict(name=name, models=models, matrices=matrices, table=table, albedo_words=words, draw_records=draw_records, overrides=overrides, materials=materials, means=means,
                instances_prefill=_pattern_bytes(ref.HEADER_BYTES + ref.INSTANCE_BYTES * (n + EXTRA), 11), bbs_prefill=_pattern_bytes(ref.BB_BYTES * (n + EXTRA), 12))


INSTANCE_CASES = tuple(str(c) for c in COUNTS) + ("alternate", "empty")


def table_bytes(table):
    return b"".join(struct.pack("<2I", int(d), int(t)) + np.asarray(mn, F32).tobytes() + np.asarray(mx, F32).tobytes() for d, t, mn, mx in table)


_instance_reference = {}


def instance_reference(name):
    """(case, instance bytes, world box bytes): computed once and shared; callers must not modify it"""
    if name not in _instance_reference:
        case = instance_case(name)
        _instance_reference[name] = (case, *ref.instance_pass(case))
    return _instance_reference[name]


# ---- the mean albedo store
def _rgba(width, height, seed, alphas=None):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 24, width * height).astype(U32)
    a = rng.integers(0, 256, width * height).astype(U32) if alphas is None else np.asarray(alphas, U32)[rng.integers(0, len(alphas), width * height)]
    return w | (a << U32(24))


def _special_alphas(width, height, seed):
    """the five alpha codes of the contract's edges on every fifth texel, random alphas between them"""
    w = _rgba(width, height, seed)
    k = np.arange(w.size)
    special = np.asarray(ALPHAS, U32)[k % 5]
    return np.where(k % 2 == 0, (w & U32(0xFFFFFF)) | (special << U32(24)), w).astype(U32)


UNUSED = 6  # the texture no draw names
MEAN_TEXTURES = (
    ("rgba 1 x 1", lambda: (_rgba(1, 1, 1, ALPHAS[3:4]), 1, 1, 1, bref.RGBA8)),
    ("rgba 3 x 5", lambda: (_special_alphas(3, 5, 2), 3, 5, 1, bref.RGBA8)),
    ("rgba 7 x 9 all 255", lambda: (np.full(63, 0xFFFFFFFF, U32), 7, 9, 1, bref.RGBA8)),
    ("rgba 64 x 64", lambda: (_special_alphas(64, 64, 3), 64, 64, 1, bref.RGBA8)),  # (at word 79: no 16-byte address)
    ("rgba 260 x 4", lambda: (_special_alphas(260, 4, 4), 260, 4, 1, bref.RGBA8)),
    ("rgba 512 x 512", lambda: (_rgba(512, 512, 5, range(128, 256)), 512, 512, 1, bref.RGBA8)),
    ("rgba 7 x 3 unused", lambda: (_rgba(7, 3, 6), 7, 3, 1, bref.RGBA8)),
    ("bc1 4 x 4 punch-through", lambda: (bc.blocks(bref.BC1, 4, 4, 1, 21, colour_order="<="), 4, 4, 1, bref.BC1)),
    ("bc1 8 x 12", lambda: (bc.blocks(bref.BC1, 8, 12, 1, 22), 8, 12, 1, bref.BC1)),
    ("bc3 4 x 4", lambda: (bc.blocks(bref.BC3, 4, 4, 1, 23), 4, 4, 1, bref.BC3)),
    ("bc3 8 x 12", lambda: (bc.blocks(bref.BC3, 8, 12, 1, 24), 8, 12, 1, bref.BC3)),
    ("bc3 5 x 7", lambda: (bc.blocks(bref.BC3, 5, 7, 1, 25), 5, 7, 1, bref.BC3)),
    ("bc5 8 x 8", lambda: (bc.blocks(bref.BC5, 8, 8, 1, 26), 8, 8, 1, bref.BC5)),
)

_mean_case = {}


def mean_case(compressed=True):
    """the store (all thirteen textures, or the seven RGBA8 ones alone: a pass record without format codes), the materials and the prefilled output"""
    if compressed not in _mean_case:
        textures = [make() for _, make in MEAN_TEXTURES if compressed or make()[4] == bref.RGBA8]
        table, words, formats = bref.pack_store(textures)
        count = table.shape[0]
        named = [t for t in range(count) if t != UNUSED]
        materials = [(t, NONE) for t in named] + [(1, 0), (NONE, 2), (count + 5, NONE)]  # the 3 x 5 texture twice; no albedo texture; an index beyond the store
        materials = np.asarray(materials, U32)
        prefill = np.full((count, 4), SENTINEL, F32)
        case = dict(table=table, words=words, formats=formats if compressed else None, materials=materials, prefill=prefill)
        case["expected"] = ref.mean_albedo_pass(table, words, case["formats"], materials, prefill)
        _mean_case[compressed] = case
    return _mean_case[compressed]
