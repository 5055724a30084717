"""numpy reference of the "drawCulling.comp" pass (DESIGN.md "Frustum culling of draws"), written from THE CULL CONTRACT's text;
csrc/kernels/draw_culling.hip implements the same contract independently and must agree bit for bit: every word of the culled draw arrays and of the counters.

Every float operation is one fp32 IEEE operation on np.float32 arrays, vectorised over the draws; sums are written out left to right as the contract brackets
them (no `@`, no np.sum, no np.dot).

The contract in short. Per draw d with a local box {lo, hi} and a matrix M (glm column-major, M[column][row]):
  corners    corner k (0 .. 7) takes hi on axis x, y, z where bit 0, 1, 2 of k is set, lo otherwise
  main view  M = mvp of transforms[draws[d].transformIndex]; c_i = ((M[0][i] x + M[1][i] y) + M[2][i] z) + M[3][i], i = x, y, z, w
  shadow     M = L_c * T, each element ((a0 b0 + a1 b1) + a2 b2) + a3 b3; c_x, c_y by the same bracketed sum over M's rows; c_w = 1 exactly
  magnitude  a = max(|lo|, |hi|) per axis with max(p, q) = p > q ? p : q; S_i = ((|M[0][i]| a.x + |M[1][i]| a.y) + |M[2][i]| a.z) + |M[3][i]|; shadow: S_w = 1
  planes     in order: near g = c_z - c_w, +x g = c_x - c_w, -x g = (-c_x) - c_w, +y g = c_y - c_w, -y g = (-c_y) - c_w (a shadow view: the last four);
             tol = max(2^-100, 2^-16 (S_a + S_w)) with max(p, q) = p > q ? p : q and S_a the magnitude of the plane's own component
  decision   outside a plane: g > tol at all eight corners (a NaN compares false); culled: outside at least one plane, counted for the first one in the order.
             Kept otherwise, a draw whose transformIndex is outside `transforms` included. The main view tests a draw only when
             ((S_x + S_y) + S_z) + S_w < 2^126 (a NaN compares false): a non-finite mvp element keeps the draw whichever component it is in
  outputs    culledDraws = draws with indexCount = 0 where culled; stats {visibleDraws, visibleTriangles (sum of indexCount // 3 of the kept draws),
             culledByPlane[5]}
"""
import numpy as np

F32 = np.float32
PLANES = ("near", "+x", "-x", "+y", "-y")
TOLERANCE_SCALE = F32(2.0 ** -16)
MAGNITUDE_LIMIT = F32(2.0 ** 126)
TOLERANCE_FLOOR = F32(2.0 ** -100)
# per plane: the component g is built from (x = 0, y = 1, z = 2) and whether it is negated
_PLANE_COMPONENT = (2, 0, 0, 1, 1)
_PLANE_NEGATED = (False, False, True, False, True)


def local_bounds(positions):
    """{lo.xyz, hi.xyz} of n x 3 float32 positions: exact fp32 minima and maxima; an empty mesh has an all-zero box"""
    p = np.asarray(positions, F32).reshape(-1, 3)
    if p.shape[0] == 0:
        return np.zeros(6, F32)
    return np.concatenate([p.min(axis=0), p.max(axis=0)]).astype(F32)


def draw_bounds(meshes_positions, draw_meshes):
    """d x 6: the local box of every draw's mesh"""
    boxes = [local_bounds(p) for p in meshes_positions]
    return np.array([boxes[m] for m in draw_meshes], F32).reshape(-1, 6)


def _component(m, i, x, y, z):
    """((M[0][i] x + M[1][i] y) + M[2][i] z) + M[3][i] for d x 16 matrices and d-vectors, one operation at a time"""
    s = m[:, 0 * 4 + i] * x
    s = s + m[:, 1 * 4 + i] * y
    s = s + m[:, 2 * 4 + i] * z
    s = s + m[:, 3 * 4 + i]
    return s


def _light_times_model(light, t):
    """rows x and y of M = L * T for d model matrices (d x 16): element [c][r] = ((L[0][r] T[c][0] + L[1][r] T[c][1]) + L[2][r] T[c][2]) + L[3][r] T[c][3];
    the other rows stay 0 (they are never read: no depth plane, and w is exactly 1)"""
    light = np.asarray(light, F32).reshape(16)
    m = np.zeros_like(t)
    for c in range(4):
        for r in range(2):
            s = light[0 * 4 + r] * t[:, c * 4 + 0]
            s = s + light[1 * 4 + r] * t[:, c * 4 + 1]
            s = s + light[2 * 4 + r] * t[:, c * 4 + 2]
            s = s + light[3 * 4 + r] * t[:, c * 4 + 3]
            m[:, c * 4 + r] = s
    return m


def _cull(draws, bounds, matrices, usable, shadow):
    """draws d x w uint32, bounds d x 6, matrices d x 16 (of the usable draws; anything elsewhere), usable d bool -> (culled draws, stats uint32[7], plane per
    draw: 0 .. 4, or 5 = kept)"""
    d = draws.shape[0]
    lo, hi = bounds[:, :3], bounds[:, 3:]
    one = np.ones(d, F32)
    with np.errstate(all="ignore"):
        al, ah = np.abs(lo), np.abs(hi)
        a = np.where(al > ah, al, ah)
        am = np.abs(matrices)
        S = [_component(am, i, a[:, 0], a[:, 1], a[:, 2]) for i in range(4)]
        if shadow:
            S[3] = one
        corners = []
        for k in range(8):
            x = hi[:, 0] if k & 1 else lo[:, 0]
            y = hi[:, 1] if k & 2 else lo[:, 1]
            z = hi[:, 2] if k & 4 else lo[:, 2]
            c = [_component(matrices, i, x, y, z) for i in range(4)]
            if shadow:
                c[3] = one
            corners.append(c)
        plane_of = np.full(d, 5, np.int64)
        if not shadow:
            usable = usable & ((((S[0] + S[1]) + S[2]) + S[3]) < MAGNITUDE_LIMIT)
        for plane in range(4, (0 if shadow else -1), -1):  # backwards, so that the first plane in the order is the one that stays
            comp = _PLANE_COMPONENT[plane]
            scaled = TOLERANCE_SCALE * (S[comp] + S[3])
            tol = np.where(TOLERANCE_FLOOR > scaled, TOLERANCE_FLOOR, scaled)  # (a NaN stays a NaN)
            outside = np.ones(d, bool)
            for c in corners:
                g = (-c[comp] if _PLANE_NEGATED[plane] else c[comp]) - c[3]
                outside &= g > tol  # (a NaN compares false)
            plane_of = np.where(outside & usable, plane, plane_of)
    culled = draws.copy()
    culled[plane_of < 5, 1] = 0
    kept = plane_of == 5
    stats = np.zeros(7, np.uint32)
    stats[0] = int(kept.sum())
    stats[1] = int((draws[kept, 1] // 3).sum()) & 0xFFFFFFFF
    for plane in range(5):
        stats[2 + plane] = int((plane_of == plane).sum())
    return culled, stats, plane_of


def _matrices_of(draws, table, first):
    """per draw the 16 floats at table[transformIndex][first : first + 16]; usable = transformIndex inside the table"""
    index = draws[:, 3].astype(np.int64)
    usable = index < table.shape[0]
    m = np.zeros((draws.shape[0], 16), F32)
    if usable.any():
        m[usable] = table[index[usable], first:first + 16]
    return m, usable


def cull_main(draws, bounds, transforms):
    """draws d x 6 uint32, bounds d x 6 float32, transforms n x 48 float32 (MainPassMatrices: mvp at floats 16 .. 31) -> dict(draws, stats, plane)"""
    draws = np.asarray(draws, np.uint32).reshape(-1, 6)
    bounds = np.asarray(bounds, F32).reshape(-1, 6)
    table = np.asarray(transforms, F32).reshape(-1, 48)
    m, usable = _matrices_of(draws, table, 16)
    culled, stats, plane = _cull(draws, bounds, m, usable, False)
    return dict(draws=culled, stats=stats, plane=plane)


def cull_shadow(draws, bounds, transforms, light):
    """draws d x 4 uint32, bounds d x 6, transforms n x 16 (the casters' model matrices), light: the cascade's 16 floats -> dict(draws, stats, plane)"""
    draws = np.asarray(draws, np.uint32).reshape(-1, 4)
    bounds = np.asarray(bounds, F32).reshape(-1, 6)
    table = np.asarray(transforms, F32).reshape(-1, 16)
    t, usable = _matrices_of(draws, table, 0)
    with np.errstate(all="ignore"):
        m = _light_times_model(light, t)
    culled, stats, plane = _cull(draws, bounds, m, usable, True)
    return dict(draws=culled, stats=stats, plane=plane)
