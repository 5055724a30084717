"""numpy reference of the alpha test of "depthPrepassRaster.comp", written from the contract text (DESIGN.md "Alpha-tested cutouts in the depth prepass";
csrc/kernels/depth_prepass_raster.hip implements the same contract independently and must agree bit for bit on all five images and all counters).

It reuses the two existing references unchanged. The alpha code of a fragment depends on (t, i, j) only, so per tested triangle: the triangle is rasterised ALONE
by prepass_raster_reference.rasterise (a one-draw copy of its draw: its fragment keys, and the motion and normal it would store at each of them),
prepass_texture_reference.sample is handed a key image that carries the triangle's global t and returns a(t, i, j) in bits 24 - 31 of its albedo word, the keys
are masked with a >= c, and the winner of a pixel is the maximum of the masked keys over all triangles. The triangles of opaque draws (c = 0) pass every
fragment, so they are rasterised together in one call in which the tested draws get an all-zero transform (their triangles keep their numbers and draw
nothing). Albedo and specular of the winners are prepass_texture_reference.sample's for the final keys; the counters are those of the whole, untested case.
"""
import numpy as np

import prepass_raster_cases as pc
import prepass_texture_reference as tref

DISCARD_ALL = 256  # what a cutoff word above 255 behaves as: min(word, 256), and no alpha code reaches 256


def cutoff_codes(cutoffs):
    return np.minimum(np.asarray(cutoffs, np.uint64).reshape(-1), DISCARD_ALL).astype(np.int64)


def _with_t(keys, t):
    """the fragment keys of a triangle rasterised alone (t = 0 there) with its number in submission order over all draws"""
    return np.where(keys != 0, (keys & np.uint64(0xFFFFFFFF00000000)) | np.uint64(t), np.uint64(0))


def render(case, tex, cutoffs, every_triangle_alone=False):
    """-> the dict of prepass_raster_reference.rasterise (keys, depth, motion, normal, albedo, specular, submitted, clipped, drawn, rejects) for an execution with
    alphaTest set, plus `fragments`: per tested triangle with a fragment a dict(t, draw, cutoff, covered (bool h x w: its fragments with zf > 0), alpha (h x w, valid
    where covered)). every_triangle_alone: the triangles of opaque draws take the per-triangle route too (the reference checked against itself)"""
    draws = np.asarray(case["draws"], np.uint32).reshape(-1, 6)
    indices = np.asarray(case["indices"], np.uint32).reshape(-1)
    codes = cutoff_codes(cutoffs)
    assert codes.size == draws.shape[0], "one cutoff per draw"
    whole = pc.rasterise(case)
    first_triangle = np.concatenate([[0], np.cumsum(draws[:, 1].astype(np.int64) // 3)])
    alone = [d for d in range(draws.shape[0]) if codes[d] != 0 or every_triangle_alone]
    # the rest: the draws that go alone keep their triangles' numbers and draw nothing, under an added all-zero transform (every clip vertex is (0, 0, 0, 0):
    # inside every plane, and w > 0 fails at the projection)
    transforms = np.asarray(case["transforms"], np.float32).reshape(-1, 48)
    nothing = draws.copy()
    nothing[alone, 3] = transforms.shape[0]
    rest = pc.rasterise(dict(case, transforms=np.concatenate([transforms, np.zeros((1, 48), np.float32)]), draws=nothing))
    keys, motion, normal = rest["keys"].copy(), rest["motion"].copy(), rest["normal"].copy()
    fragments = []
    for d in alone:
        for local in range(int(draws[d, 1]) // 3):
            t = int(first_triangle[d]) + local
            row = draws[d].astype(np.int64)
            row[0], row[1] = row[0] + 3 * local, 3
            if row[0] + 3 > indices.size:
                continue  # outside its buffer: a counted reject of the whole case, no fragment
            single = pc.rasterise(dict(case, draws=row.astype(np.uint32).reshape(1, 6)))
            own = _with_t(single["keys"], t)
            covered = own != 0
            if not covered.any():
                continue
            alpha = tref.sample(case, tex, own)["albedo"] >> np.uint32(24)
            kept = covered & (alpha.astype(np.int64) >= codes[d])
            fragments.append(dict(t=t, draw=d, cutoff=int(codes[d]), covered=covered, alpha=alpha))
            better = kept & (own > keys)
            keys[better], motion[better], normal[better] = own[better], single["motion"][better], single["normal"][better]
    out = dict(keys=keys, depth=(keys >> np.uint64(32)).astype(np.uint32).view(np.float32), motion=motion, normal=normal, fragments=fragments)
    s = tref.sample(case, tex, keys)
    out.update(albedo=s["albedo"], specular=s["specular"])
    out.update({name: whole[name] for name in ("submitted", "clipped", "drawn", "rejects")})
    return out


def winner_draw(case, keys):
    """the draw of each pixel's winner, -1 for the sky"""
    draws = np.asarray(case["draws"], np.uint32).reshape(-1, 6)
    first_triangle = np.concatenate([[0], np.cumsum(draws[:, 1].astype(np.int64) // 3)])
    t = (np.asarray(keys, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return np.where(keys != 0, np.searchsorted(first_triangle, t, side="right") - 1, -1)
