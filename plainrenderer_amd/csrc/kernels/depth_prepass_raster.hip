// "depthPrepassRaster.comp": the depth prepass as a compute pass - RenderFrontend::renderDepthPrepass (RenderFrontend.cpp:351, 792-802; pass description
// :1717-1735; depthPrepass.vert / depthPrepass.frag) for opaque meshes with one constant material per draw: the current frame's depth (Depth32), motion
// (RG16_sNorm), world-space normal, albedo and specular (RGBA8) in one execution. One kernel family serves both math modes: every decision is an integer one.
// PLR_BUILD_FLAGS: -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt
//
// THE RASTERISATION CONTRACT (DESIGN.md "Depth prepass as a compute pass"; tests/prepass_raster_reference.py implements it independently and all five images and
// all counters must agree bit for bit). fp32 IEEE, no contraction, correctly rounded divide and sqrt, except where fp64 (IEEE, no contraction) is named.
// A draw {firstIndex, indexCount, vertexOffset, transformIndex, albedo, specular} submits indexCount / 3 triangles (rounded down); triangle t is the t-th in
// submission order over all draws. transforms[transformIndex] = {model, mvp, mvpPrevious}, glm column-major.
//   outside a buffer: a triangle is a counted reject and draws nothing when its three index slots are not all inside `indices`, when a vertex (index +
//     vertexOffset, in 64 bits) is not inside `positions` AND `normals`, or when transformIndex is not inside `transforms`
//   clip = mvp * (p, 1), four components, each m[0][i] x + m[1][i] y + m[2][i] z + m[3][i] summed left to right. A triangle with a non-finite clip
//     component is a counted reject.
//   clipping, Sutherland-Hodgman, five planes in this order with d(v) = w - z (near; reverse Z, depth clamp off), 32 w - x, 32 w + x, 32 w - y, 32 w + y (32 w
//     is one multiply). A vertex is inside when d >= 0. The polygon starts as (v0, v1, v2); for every plane, for i = 0 .. n - 1 with a = poly[i],
//     b = poly[(i + 1) mod n]: a is emitted when it is inside; when exactly one of a, b is inside, the vertex on the edge is emitted behind it, always computed
//     from the inside vertex I towards the outside vertex O: t = d_I / (d_I - d_O), v = I + t (O - I) per component (x, y, z, w). Two triangles that share an
//     edge get the identical vertex. The output of plane k (0 .. 4) holds at most 4 + k vertices; what rounding might produce beyond that is dropped. A
//     triangle counts as clipped when any of its polygon's vertices was outside any plane. A polygon of fewer than 3 vertices draws nothing; otherwise it is
//     fanned from its first vertex: sub-triangle k = (poly[0], poly[k + 1], poly[k + 2]), at most 6. The far plane is a per-fragment rule (below).
//   per sub-triangle vertex: it must have w > 0; ndc = (x / w, y / w), z = clip.z / w; xf = (ndc.x * 0.5 + 0.5) * width, yf = (ndc.y * 0.5 + 0.5) * height,
//     no Y flip; |xf| and |yf| must be < 2^20 and z finite (a NaN fails). A sub-triangle with a vertex that fails is a counted reject.
//   X = rint(xf * 256), Y = rint(yf * 256), int32. A = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0) in int64. Cull mode Back with a counter-clockwise front face
//     (:1729, VulkanPipeline.cpp:61): only A < 0 is drawn. Such a sub-triangle is rasterised as (v0, v2, v1) - area -A > 0 - by the shadow contract word for
//     word: pixel box (Xmin + 127) >> 8 .. (Xmax - 128) >> 8 clipped to the image (an empty box: not drawn, not counted), edge functions in int64 at the pixel
//     centres (256 i + 128, 256 j + 128), the top-left rule, l1 = float(E_20) / float(A'), l2 = float(E_01) / float(A'), zf = (z0 + l1 (z1' - z0)) + l2 (z2' - z0)
//     with 1' = 2 and 2' = 1. Every sub-triangle with a non-empty box counts as drawn.
//   a fragment is kept when zf > 0 (a NaN and everything at or beyond the far plane is dropped: depth 0 is the sky's code); it is not clamped
//   visibility: attachments cleared to 0, depth test GreaterEqual, depth write on (:1726-1727), primitives in order: a pixel's winner is the MAXIMUM of the
//     64-bit keys (bits(zf) << 32) | t of its fragments. All sub-triangles of one triangle share t; of two fragments at bit-equal depth the later t wins.
//   a pixel without a fragment gets depth 0, motion (0, 0), and 0 in all four channels of normal, albedo and specular. Every texel of all five images is written
//     by every execution: the clear is part of the pass.
//   attributes of the winner, once per pixel (i, j), from the ORIGINAL triangle, in fp64: P = ((2 i + 1) / width - 1, (2 j + 1) / height - 1, 1), V_k = the fp32
//     clip (x, y, w) of original vertex k promoted; det(A, B, C) = (A.x (B.y C.w - B.w C.y) - A.y (B.x C.w - B.w C.x)) + A.w (B.x C.y - B.y C.x);
//     e0 = det(P, V1, V2), e1 = det(P, V2, V0), e2 = det(P, V0, V1); s = (e0 + e1) + e2; b_k = e_k / s; s zero or non-finite: b = (1, 0, 0).
//     Sums over k below are (b0 a0 + b1 a1) + b2 a2.
//   normal: the stored vertex normal, or where all three of its components are 0 (a mesh given without normals) the face normal normalize(cross(p0 - p2,
//     p0 - p1)) of the model-space positions, fp64; N_k = normalize(mat3(model) * normal_k), component r = (m[0][r] x + m[1][r] y) + m[2][r] z; n = normalize(
//     sum b_k N_k); every normalize is v / sqrt((x x + y y) + z z), and (0, 0, 0) where that length is not a finite number > 0. n is rounded once to fp32, then
//     n * 0.5 + 0.5 (fp32, two operations) is stored by the image contract's UNORM8 rule with alpha 255; a zero n therefore stores 128, 128, 128.
//   motion (.frag:34-40): ndcCurrent = P.xy + currentFrameCameraJitter (the pixel centre, not passPos.xy / passPos.w: the same in real arithmetic);
//     prev_k = mvpPrevious * (p_k, 1) in fp32 as above, promoted; ndcPrevious = (sum b_k prev_k.x, sum b_k prev_k.y) / sum b_k prev_k.w + previousFrameCameraJitter;
//     m = (ndcPrevious - ndcCurrent) * 0.5, rounded to fp32; code = rint(fmin(fmax(m, -1), 1) * 32767) as int16, 0 for a NaN. A previous w sum that is not a
//     finite number > 0 stores (0, 0). Both jitters come from the global UBO.
//   albedo, specular: the two RGBA8 words of the winner's draw, or for a draw that names a texture the sampled texel (THE SAMPLING CONTRACT below).
//   counters: submitted (triangles of all draws), clipped, drawn (sub-triangles), rejects (triangles and sub-triangles, as above).
//   depthPrepass.frag's alpha test (:27-30): THE ALPHA TEST CONTRACT below; without it all meshes are opaque.
//
// THE SAMPLING CONTRACT (DESIGN.md "Material textures in the depth prepass"; tests/prepass_texture_reference.py implements it independently, bit for bit). Only
// an execution whose third push-constant word textureCount is > 0 samples, and only the albedo and specular words of a winner pixel change; visibility, depth,
// motion, normal and the counters do not. fp64 IEEE without contraction where named, fp32 IEEE elsewhere.
//   texture store: `texels` holds uint32 RGBA8 texels, R in the low byte: all textures, each with all its levels back to back and unpadded; level l is row-major
//     W_l x H_l with W_l = max(1, W_0 >> l), H_l likewise. `textures` holds {texelOffset (in texels), width, height, mipCount} per texture; an entry is usable when
//     1 <= width, height <= 16384 and 1 <= mipCount <= floor(log2(max(width, height))) + 1. `materials` holds {albedoTexture, specularTexture} per draw, 0xffffffff
//     = none. A word that is none, is >= textureCount or names an unusable entry makes that output the draw's constant word. A texel whose 64-bit address is
//     outside `texels` reads 0.
//   uv: `uvs` holds 2 floats per vertex, indexed like positions; a vertex outside `uvs` has (0, 0). u(P) = (b0 u0 + b1 u1) + b2 u2 in fp64 with the b of the
//     pixel centre P, v likewise. If u or v is not finite or |.| >= 2^20, both are taken as 0 for the taps.
//   derivatives, without a quad or a neighbouring pixel's triangle: the same triangle's b by the same formula ((1, 0, 0) fallback included) at
//     P_x = ((2 (i + 1) + 1) / width - 1, P.y, 1) and P_y = (P.x, (2 (j + 1) + 1) / height - 1, 1). Per texture with its W_0, H_0 as fp64:
//     ax = ((u(P_x) - u(P)) W_0, (v(P_x) - v(P)) H_0) from the raw u, v (before the validity rule), ay likewise with P_y; rx = ax.x^2 + ax.y^2, ry likewise;
//     rho2 = rx > ry ? rx : ry, exactly that expression.
//   level, fp32: r = (float)rho2; lod = 0.5f det_log2f(r) + g_mipBias; where !(lod > 0), lod = 0 (also a NaN); where lod > mipCount - 1, lod = that;
//     q = (int)floorf(lod * 256.f + 0.5f), L0 = q >> 8, fw = q & 255, L1 = min(L0 + 1, mipCount - 1).
//   taps, in integers (8 sub-texel bits), per level with dimensions (W, H): Tu = (int64)floor((u W - 0.5) 256 + 0.5) in fp64; x0 = Tu >> 8 (arithmetic),
//     fx = Tu & 255, x1 = x0 + 1, both wrapped to [0, W) by a non-negative modulo (repeat); y0, fy, y1 likewise with v and H. Per channel
//     S_l = (256 - fx)(256 - fy) c00 + fx (256 - fy) c10 + (256 - fx) fy c01 + fx fy c11; S = (256 - fw) S_L0 + fw S_L1 (<= 255 * 2^24: fits uint32); the stored
//     code is (S + 2^23 - 1 + ((S >> 24) & 1)) >> 24, round half even. All four channels, alpha included; albedo is filtered in code space.
//   Without the seventh push-constant word isotropic trilinear filtering stands in for the reference's anisotropic sampler; with it: THE ANISOTROPIC CONTRACT
//   below, whose probe placement and count are this project's (Vulkan leaves them to the implementation). The normal map: THE NORMAL MAP CONTRACT below.
//
// THE ALPHA TEST CONTRACT (DESIGN.md "Alpha-tested cutouts in the depth prepass"; tests/prepass_alpha_reference.py implements it independently, bit for bit). Only an
// execution whose fourth push-constant word alphaTest is != 0 tests (it needs textureCount > 0 and storage buffer 10 `alphaCutoffs`, one uint32 per draw).
//   per-draw cutoff: draw d has the cutoff code c = min(alphaCutoffs[d], 256). c = 0 is opaque; the reference's alpha < 0.5 -> discard is c = 128 (a / 255 < 0.5 <=>
//     a <= 127); a word above 255 gives c = 256, which no alpha code reaches: every fragment of the draw is discarded (255 keeps a = 255).
//   alpha of a fragment: a fragment of triangle t at pixel (i, j) has the alpha code a(t, i, j) = bits 24 - 31 of exactly the albedo word the sampling contract
//     yields for triangle t at that pixel: the same b at P, P_x, P_y from the ORIGINAL triangle, the same UV validity rule, level selection with g_mipBias, taps
//     and round-half-even; for a draw whose albedo material word names no usable texture, bits 24 - 31 of the draw's constant albedo word. It depends on (t, i, j)
//     only - not on the sub-triangle of the clipped fan that produced the fragment, nor on any other fragment.
//   visibility: a pixel's winner is the maximum key over its fragments that pass coverage, the zf > 0 rule and a(t, i, j) >= c: one clause added to the visibility
//     rule above, nothing else of it changes. A pixel whose fragments all fail is sky (depth 0, all images 0). Depth, motion, normal, albedo and specular of a
//     winner are computed as before; consequently every winner pixel of a draw has a stored albedo.a >= c. The four counters do not depend on alpha: drawn still
//     counts sub-triangles with a non-empty box.
//   freedom for the kernel: the result is a maximum, so a kernel may skip the alpha evaluation of a fragment whose key is not above the cell's current value; the
//     image does not change. (There is no counter of discarded fragments: it would forbid exactly that.)
//   sunShadow.frag's alpha test is not part of this pass: the shadow casters are another mesh set with UVs, textures and cutoffs of their own
//   (kernels/sun_shadow_raster.hip, THE CUTOUT CONTRACT; plrf_set_shadow_caster_cutouts).
//
// THE NORMAL MAP CONTRACT (DESIGN.md "Normal maps in the depth prepass"; tests/prepass_normal_reference.py implements it independently, bit for bit on every texel
// of shadingNormal). Only an execution whose fifth push-constant word normalMap is 1 or 2 writes storage image 5, shadingNormal (it needs textureCount > 0 and
// storage buffers 11 - 13); visibility, depth, motion, normal, albedo, specular and the counters do not depend on it. fp64 IEEE without contraction, correctly
// rounded divide and sqrt, unless stated otherwise.
//   inputs: `tangents` and `bitangents` hold 3 floats per vertex, indexed like positions; a vertex outside `tangents` has the tangent (0, 0, 0), one outside
//     `bitangents` the bitangent (0, 0, 0). `normalMaterials` holds one uint32 per draw: an index into the SAME textures / texels store as albedo and specular, or
//     0xffffffff; usable by the sampling contract's rule. `materials` keeps its 8-byte stride.
//   per winner pixel of triangle t at P, with the b of the ORIGINAL triangle:
//     per-vertex basis: T_k = normalize(mat3(model) * tangent_k), B_k likewise, by the normal rule's arithmetic word for word (component r = (m[0][r] x +
//       m[1][r] y) + m[2][r] z; normalize gives (0, 0, 0) where the length is not a finite number > 0); N_k is exactly the normal rule's, face normal included.
//     interpolated basis: T = sum b_k T_k, B = sum b_k B_k, Nv = sum b_k N_k, each (b0 a0 + b1 a1) + b2 a2; NOT renormalised (passTBN is interpolated raw).
//     texel: the sampling contract's RGBA8 word for the draw's normal texture at this pixel (same UV, validity rule, derivatives, level with g_mipBias, taps, round
//       half even: uvSampleAt, sampleTexture); cx = bits 0 - 7, cy = bits 8 - 15; x = cx / 255.0, y = cy / 255.0.
//     decode 1, reference (triangle.frag:181-182, as written): z = sqrt(((1 - x x) + y) + y), n_t = (2 x - 1, 2 y - 1, 2 z - 1); the radicand is never negative.
//     decode 2, unit: nx = 2 x - 1, ny = 2 y - 1, q = (1 - nx nx) - ny ny, nz = q > 0 ? sqrt(q) : 0, n_t = (nx, ny, nz).
//     shading normal: M_r = (T_r n_t.x + B_r n_t.y) + Nv_r n_t.z, n_s = normalize(M) with the zero rule; where n_s is zero it is the normal rule's n (the word of
//       `normal`; the reference's NaN fallback N = passTBN[2], :194-196, normalised). n_s is rounded once to fp32 and stored as n_s * 0.5 + 0.5 by the UNORM8 rule,
//       alpha 255.
//     no normal map: the pixel stores exactly the word the pass stores to `normal` - a draw whose normalMaterials word names no usable texture, a draw at or past
//       drawCount, a draw past the end of normalMaterials.
//   a pixel without a winner stores 0; every texel of shadingNormal is written by every normal-mapped execution.
//   deviations: the filtered texel is quantised to 8 bits before the decode; isotropic trilinear filtering, or the anisotropic contract's probes; fp32 tangents for the A2R10G10B10 SNORM vertex format;
//     the normalised fallback; decode 1 is the reference's expression, not a unit-length one.
// The tile kernel of such an execution (kNormalMap) leaves the winner's t, or kNoWinner, in the shadingNormal texel, and depthPrepassShadingNormalKernel behind it,
// a lane per pixel, turns that texel into the shading normal in place.
//
// THE BLOCK DECODE CONTRACT (DESIGN.md "Block-compressed textures in the depth prepass"; tests/prepass_bc_reference.py implements it independently, bit for bit). Only
// an execution whose sixth push-constant word textureFormats is 1 decodes (it needs textureCount > 0 and storage buffer 14 `textureFormats`, one uint32 per texture);
// a push of 20 bytes or fewer, or the word at 0, is the pass above. Everything is in integers; / is floor division of non-negative integers.
//   format codes: 0 RGBA8, as above; 1 BC1, 8-byte blocks; 2 BC3, 16-byte blocks; 3 BC5, 16-byte blocks.
//   layout: level l of a compressed texture is ceil(W_l / 4) x ceil(H_l / 4) blocks, row-major, W_l = max(1, W_0 >> l) as before; levels lie back to back and
//     unpadded, in the same `texels` buffer as the RGBA8 textures. texelOffset of a compressed entry counts uint32 words of `texels` (for RGBA8, words and texels are
//     the same number). Texel (x, y) of a level lives in block (x >> 2, y >> 2) at position i = 4 (y & 3) + (x & 3). Levels smaller than 4 x 4 are one block; the
//     positions outside the level are never addressed.
//   colour block (8 bytes): c0, c1 little-endian uint16 RGB565, red in the high bits, then a little-endian uint32 of 2-bit indices, texel i at bits 2 i. Expansion:
//     r8 = (r5 << 3) | (r5 >> 2), g8 = (g6 << 2) | (g6 >> 4), b8 like r8. Four-colour mode, per channel: index 0 is c0, 1 is c1, 2 is (2 c0 + c1 + 1) / 3, 3 is
//     (c0 + 2 c1 + 1) / 3. Three-colour mode: 0 and 1 as before, 2 is (c0 + c1 + 1) >> 1, 3 is (0, 0, 0). BC1 uses four-colour mode when c0 > c1, compared as uint16,
//     otherwise three-colour mode; BC1 alpha is always 255, index 3 of three-colour mode included (the reference's BC1_RGB variant). BC3's colour block is always
//     four-colour mode, whatever the order of c0 and c1.
//   alpha block (8 bytes: BC3's first half and both halves of BC5): bytes a0, a1, then a little-endian 48-bit integer of 3-bit indices, texel i at bits 3 i. Indices 0
//     and 1 are a0 and a1. With a0 > a1, index k = 2 .. 7 is ((8 - k) a0 + (k - 1) a1 + 3) / 7; otherwise k = 2 .. 5 is ((6 - k) a0 + (k - 1) a1 + 2) / 5, 6 is 0
//     and 7 is 255. Both divisions round to nearest and have no ties.
//   words, R in the low byte: BC1 (r, g, b, 255); BC3: bytes 0 - 7 the alpha block, 8 - 15 the colour block: (r, g, b, a); BC5: bytes 0 - 7 the R block, 8 - 15 the G
//     block: (R, G, 0, 255).
//   usable entries: a compressed entry is usable under the sampling contract's rule on width, height and mipCount; in addition its texelOffset must be a multiple of 2
//     words (BC1) or 4 words (BC3, BC5). An entry whose format code is above 3 is unusable. An unusable entry yields the draw's constant word, as before.
//   out of range: a tap whose block does not lie wholly inside `texels` reads word 0, all four channels; the 64-bit address is checked before the load.
//   everything else is the sampling contract, unchanged and applied to the decoded words: UV, the forward-difference derivatives, the level from W_0, H_0 in texels,
//     the taps, repeat wrap and weights, the round-half-even code.
// The format-aware instantiations (kFormats) decode per tap: blockTexel loads the tap's block with one plain vector load and extracts its texel; the alpha-only
// path (kFirst == 3) loads BC3's alpha block alone and nothing for BC1 and BC5.
//
// THE ANISOTROPIC CONTRACT (DESIGN.md "Anisotropic filtering in the depth prepass"; tests/prepass_aniso_reference.py implements it independently, bit for bit). Only an
// execution whose seventh push-constant word maxAnisotropy = A is 2 .. 16 runs it (it needs textureCount > 0; a push of 24 bytes or fewer, or the word at 0 or 1, is
// the pass above; a value above 16 is refused). It applies to EVERY sample: albedo, specular, the alpha of the coverage path, the normal-map texel, RGBA8 and
// block-compressed alike. Everything not named is the sampling contract. fp64 IEEE without contraction where values are fp64, integers elsewhere.
//   major axis: per texture and pixel ax, ay, rx, ry as above. The major axis is x where rx > ry (the rho2 expression), otherwise y; rmax = rho2, rmin the other of
//     rx, ry; (du, dv) are the raw forward differences of the major axis: (dudx, dvdx) or (dudy, dvdy).
//   probe count: N = 1; while (N < A && (double)(N N) rmin < rmax) N++. No square root, no division. A NaN compares false: N = 1; rmin = 0 < rmax: N = A; rmax = 0: N = 1.
//   level: r = (float)(rho2 / (double)(N N)), then lod, the clamps, q, L0, L1, fw as above (N = 1 divides by 1.0: the level is the isotropic one).
//   probes: N = 1: the one probe is (u, v) as validated above, no arithmetic on it. N > 1, k = 0 .. N - 1: t_k = (double)(2 k + 1 - N) / (double)(2 N),
//     u_k = u + t_k du, v_k = v + t_k dv - a multiply, then an add, from the RAW u, v - and the validity rule anew per probe: u_k or v_k not finite or |.| >= 2^20:
//     that probe taps at (0, 0).
//   sum: per probe the trilinear integer sum per channel S_k = (256 - fw) S_L0 + fw S_L1 <= 255 * 2^24 at the shared L0, L1, fw; T = sum S_k in 64 bits, T < 2^36.
//   stored code: T / (N 2^24) rounded half to even: D = N 2^24, qd = T / D, rem = T - qd D, code = qd + (2 rem > D || (2 rem == D && (qd & 1))); all four channels.
//     For N = 1 this is (S + 2^23 - 1 + ((S >> 24) & 1)) >> 24.
// The anisotropic instantiations (kAniso) exist in the format-aware form only: four tile kernels and one shading-normal kernel; without binding 14 their `formats`
// pointer is null and every texture has format code 0. The kernel counts N without the early exit (the test is monotone in n: sampleTexture), walks one rolled loop of
// N or 2 N steps - a step is one (probe, level) pair, so one copy of the taps serves both levels and L1's steps do not exist where fw == 0 - to each lane's own
// count, and divides by a truncated fp32 quotient that is exact for T >> 24 < 2^12 and N <= 16.
//
// THE TILE WINDOW (DESIGN.md "Rasterising in a partition"; tests/test_prepass_window.py). A push of 44 bytes - words 0 - 6 as above, 0 where a feature is off, then
// {windowTileX0, windowTileY0, windowTileX1, windowTileY1}, half-open, in 64 x 64 tiles of the bound images - restricts the execution to the pixels of those tiles:
// every texel of the five images (and of shadingNormal) inside the window gets exactly the bits of the unwindowed execution - snapping, coverage, keys, attributes
// and samples are computed in full-frame coordinates -, no kernel stores to a texel outside it, and the four counters do not depend on it. Every shorter record is
// the whole grid. Refused: an empty or inverted window, one that reaches past the tile grid, a push size that is none of 8, 12, 16, 20, 24, 28, 44. The tile
// kernel's grid is the window's tiles (a block's tile is blockIdx + the window's origin), the shading-normal kernel's the window's columns and rows; set-up counts
// every sub-triangle with a non-empty box as drawn but appends a record only where its tile rectangle meets the window.
//
// Two kernels. SET-UP: a lane per triangle finds its draw (block-wide prefix sum, LDS bisection), transforms, clips (the polygon lives in LDS, a column per lane),
// projects, snaps, culls and boxes; the block's sub-triangles are appended through one 64-bit atomic per block to a dense array of 4-byte tile rectangles and an
// array of records that carry t. TILES: a 256-thread block per 64 x 64 tile keeps the tile's 64-bit keys in LDS (32 KB); each wave reads 256 rectangles per step
// and queues those that touch its tile; a hit whose box inside the tile is at most 4 x 4 pixels is rasterised by its lane, larger ones by the whole wave in
// 8 x 8 stamps, in int32 where the triangle is narrow; LDS 64-bit atomic max. RESOLVE: behind the barrier a lane per pixel finds the winner's draw, fetches its
// three vertices, evaluates the fp64 attributes and stores the five images, a wave per row segment of 64 four-byte texels (256 contiguous bytes per image).
// Every tile scans every rectangle: no bins in this version. No global atomics on the targets. The tile kernel is a template over kTextured: the launcher picks
// the instantiation by textureCount, and only the textured one holds the sampling code. Its resolve fetches the winner's vertices once for the three barycentric
// evaluations, samples nothing for a draw without a usable texture, and computes every texel, UV and table address in 64 bits and checks it against its buffer
// before the load. A third instantiation (kTextured && kAlphaTest, picked by alphaTest) holds the alpha test: per step of 64 records every lane finds its
// record's draw, cutoff, texture, V_k and UVs - once per record, all 64 chains of loads at once - and leaves them in LDS; a record of an opaque draw takes the path
// it takes in the other two; the lane path and the wave path of a tested record queue the fragments whose key is above their cell (the early out), and the wave
// samples 64 queued fragments at a time, one per lane. That kernel takes all its arguments from LDS.
// The draw lookup and the step from three snapped vertices to a record are device/raster_setup.h's, the scan, the walk and a fragment's coverage and depth
// device/raster_tile_walk.h's, both shared with "sunShadowRaster.comp"; the clip planes, clipComponent and the step from a clipped vertex to the sub-pixel grid device/raster_clip.h's, shared
// with "debugGeometry.comp"; this file holds the polygon clip, the block's append, what becomes of a fragment (the key, the
// alpha test's queue), the resolve and the launcher.
#include <algorithm>

#include "../backend.h"
#include "../device/bc_decode.h"
#include "../device/depth_prepass_raster.h"
#include "../device/detmath.h"
#include "../device/raster_clip.h"
#include "../device/raster_setup.h"
#include "../device/raster_tile_walk.h"

namespace plr {
namespace prepass {

using rastercov::EdgeSteps;
using rastercov::kNarrowFlag;
using rastercov::SetupRecord;

struct SetupParams {
    const float* transforms; const float* positions; const uint32_t* indices; const Draw* draws;
    ScratchHeader* header; TriangleOrigin* origins; uint32_t* rects; Record* records;
    uint32_t drawCount, triangleCount, capacity, transformCount, vertexCount, indexCount;
    int32_t width, height;
    uint32_t window; // the tile window in a tile rectangle's form: first tile x | first tile y << 8 | last tile x << 16 | last tile y << 24 (the whole grid without a window)
};
// do two tile rectangles (inclusive, four bytes) share a tile?
PLR_DI bool rectanglesMeet(uint32_t a, uint32_t b) {
    return (a & 255u) <= ((b >> 16) & 255u) && (b & 255u) <= ((a >> 16) & 255u) && ((a >> 8) & 255u) <= (b >> 24) && ((b >> 8) & 255u) <= (a >> 24);
}

// one Sutherland-Hodgman step of this lane's polygon: src (n vertices) -> dst (at most `cap`), both LDS arrays [slot * 4 + component][thread]
PLR_DI int clipPolygon(const float (*src)[256], int n, float (*dst)[256], int cap, int plane, uint32_t tid, bool& changed) {
    int m = 0;
    for (int i = 0; i < n; i++) {
        const int j = i + 1 == n ? 0 : i + 1;
        const float ax = src[i * 4 + 0][tid], ay = src[i * 4 + 1][tid], az = src[i * 4 + 2][tid], aw = src[i * 4 + 3][tid];
        const float bx = src[j * 4 + 0][tid], by = src[j * 4 + 1][tid], bz = src[j * 4 + 2][tid], bw = src[j * 4 + 3][tid];
        const float da = planeDistance(plane, ax, ay, az, aw), db = planeDistance(plane, bx, by, bz, bw);
        const bool ina = da >= 0.f, inb = db >= 0.f;
        if (!ina) changed = true;
        if (ina && m < cap) {
            dst[m * 4 + 0][tid] = ax; dst[m * 4 + 1][tid] = ay; dst[m * 4 + 2][tid] = az; dst[m * 4 + 3][tid] = aw;
            m++;
        }
        if (ina != inb && m < cap) { // from the inside vertex towards the outside one
            const float ix = ina ? ax : bx, iy = ina ? ay : by, iz = ina ? az : bz, iw = ina ? aw : bw;
            const float ox = ina ? bx : ax, oy = ina ? by : ay, oz = ina ? bz : az, ow = ina ? bw : aw;
            const float di = ina ? da : db, dout = ina ? db : da;
            const float t = di / (di - dout);
            dst[m * 4 + 0][tid] = ix + t * (ox - ix); dst[m * 4 + 1][tid] = iy + t * (oy - iy);
            dst[m * 4 + 2][tid] = iz + t * (oz - iz); dst[m * 4 + 3][tid] = iw + t * (ow - iw);
            m++;
        }
    }
    return m;
}

// sub-triangle (0, k + 1, k + 2) of the projected polygon in `poly` ({X, Y as int bits, z, ok}): 0 nothing, 1 a reject, 2 a record (with its tile rectangle)
PLR_DI int setupSubTriangle(const float (*poly)[256], int k, uint32_t tid, int32_t width, int32_t height, SetupRecord* rec, uint32_t* rect) {
    const int slot[3] = {0, k + 2, k + 1}; // vertices 1 and 2 exchanged: a front face (A < 0) has A' = -A > 0
    int32_t X[3], Y[3];
    float z[3];
    bool ok = true;
    for (int v = 0; v < 3; v++) {
        X[v] = (int32_t)f2u(poly[slot[v] * 4 + 0][tid]); Y[v] = (int32_t)f2u(poly[slot[v] * 4 + 1][tid]);
        z[v] = poly[slot[v] * 4 + 2][tid];
        ok = ok && f2u(poly[slot[v] * 4 + 3][tid]) != 0u;
    }
    if (!ok) return 1;
    return rastercov::setupTriangle(X, Y, z, width, height, rec, rect) ? 2 : 0;
}

__global__ __launch_bounds__(256) void depthPrepassSetupKernel(SetupParams p) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, tid = threadIdx.x;
    // the lane's polygon, [slot * 4 + component][thread]: planes 0, 2 and 4 write polyA (at most 4, 6, 8 vertices), the input and planes 1 and 3 polyB (3, 5, 7)
    __shared__ float polyA[32][256];
    __shared__ float polyB[28][256];
    const uint32_t wave = threadIdx.x >> 6;
    const rastercov::TriangleSlot found = rastercov::drawOfTriangle(p.draws, p.drawCount, p.triangleCount, t);
    uint32_t rejects = 0;
    bool clipped = false;
    int n = 0; // vertices of the clipped and projected polygon in polyA
    if (found.found) {
        p.origins[t] = TriangleOrigin{found.draw, found.local};
        const Draw draw = p.draws[found.draw];
        const uint64_t at = (uint64_t)draw.firstIndex + (uint64_t)found.local * 3u;
        bool inBuffers = at + 3u <= (uint64_t)p.indexCount && draw.transformIndex < p.transformCount;
        uint64_t v[3] = {0, 0, 0};
        if (inBuffers)
            for (int k = 0; k < 3; k++) {
                v[k] = (uint64_t)p.indices[at + k] + (uint64_t)draw.vertexOffset;
                inBuffers = inBuffers && v[k] < (uint64_t)p.vertexCount;
            }
        if (!inBuffers) rejects = 1;
        else {
            const float* M = p.transforms + (size_t)draw.transformIndex * 48u + 16u; // mvp
            bool finite = true;
            for (int k = 0; k < 3; k++) {
                const float* q = p.positions + v[k] * 3u;
                const float x = q[0], y = q[1], z = q[2];
                for (int i = 0; i < 4; i++) {
                    const float c = clipComponent(M, i, x, y, z);
                    finite = finite && fabsf(c) < __builtin_inff(); // (a NaN fails the comparison)
                    polyB[k * 4 + i][tid] = c;
                }
            }
            if (!finite) rejects = 1;
            else {
                n = clipPolygon(polyB, 3, polyA, 4, 0, tid, clipped);
                n = clipPolygon(polyA, n, polyB, 5, 1, tid, clipped);
                n = clipPolygon(polyB, n, polyA, 6, 2, tid, clipped);
                n = clipPolygon(polyA, n, polyB, 7, 3, tid, clipped);
                n = clipPolygon(polyB, n, polyA, 8, 4, tid, clipped);
                if (n < 3) n = 0;
                const float wf = (float)p.width, hf = (float)p.height;
                for (int i = 0; i < n; i++) { // project in place: {X, Y (int bits), z, ok}
                    const float x = polyA[i * 4 + 0][tid], y = polyA[i * 4 + 1][tid], z = polyA[i * 4 + 2][tid], w = polyA[i * 4 + 3][tid];
                    int32_t X, Y;
                    float nz;
                    const bool ok = projectAndSnap(x, y, z, w, wf, hf, &X, &Y, &nz);
                    polyA[i * 4 + 0][tid] = u2f((uint32_t)X);
                    polyA[i * 4 + 1][tid] = u2f((uint32_t)Y);
                    polyA[i * 4 + 2][tid] = nz;
                    polyA[i * 4 + 3][tid] = u2f(ok ? 1u : 0u);
                }
            }
        }
    }
    // pass 1: which sub-triangles survive (they count as drawn), and which of those get a record: the ones whose tile rectangle meets the window
    uint32_t surviveMask = 0, drawnMine = 0;
    for (int k = 0; k + 2 < n; k++) {
        SetupRecord unused;
        uint32_t rect = 0;
        const int what = setupSubTriangle(polyA, k, tid, p.width, p.height, &unused, &rect);
        if (what == 1) rejects++;
        if (what == 2) {
            drawnMine++;
            if (rectanglesMeet(rect, p.window)) surviveMask |= 1u << k;
        }
    }
    const uint32_t mine = (uint32_t)__popc(surviveMask);
    // one 64-bit atomic per block hands it a run of slots (the low word is the cursor) and counts its triangles (the high word); a lane appends 0 .. 6
    // records, so the block's prefix sum is over counts (the shadow pass appends one survivor per lane by ballot; neither form serves the other)
    // the drawn count rides in the prefix sum's high half: a wave appends at most 384 records and draws at most 384 sub-triangles, a block four times as many
    __shared__ uint32_t waveSurvivors[4], blockFound, blockRejects, blockClipped, blockBase;
    if (threadIdx.x == 0) blockFound = blockRejects = blockClipped = 0u;
    uint32_t incl = mine | (drawnMine << 16);
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
        if ((int)lane >= off) incl += up;
    }
    if (lane == 63u) waveSurvivors[wave] = incl;
    __syncthreads();
    const unsigned long long foundMask = __ballot(found.found), clippedMask = __ballot(clipped);
    if (lane == 0) { atomicAdd(&blockFound, (uint32_t)__popcll(foundMask)); atomicAdd(&blockClipped, (uint32_t)__popcll(clippedMask)); }
    if (rejects) atomicAdd(&blockRejects, rejects);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t both = waveSurvivors[0] + waveSurvivors[1] + waveSurvivors[2] + waveSurvivors[3];
        const uint32_t survivors = both & 0xffffu, blockDrawn = both >> 16;
        const unsigned long long old = atomicAdd((unsigned long long*)&p.header->cursor, (unsigned long long)survivors | ((unsigned long long)blockFound << 32));
        blockBase = (uint32_t)old;
        if (blockRejects) atomicAdd(&p.header->rejects, blockRejects);
        if (blockClipped) atomicAdd(&p.header->clipped, blockClipped);
        if (blockDrawn) atomicAdd(&p.header->drawn, blockDrawn); // (not the cursor: a window drops records, the counter does not depend on it)
    }
    __syncthreads();
    uint32_t slot = blockBase + (incl & 0xffffu) - mine;
    for (uint32_t w = 0; w < wave; w++) slot += waveSurvivors[w] & 0xffffu;
    // pass 2: the records
    for (int k = 0; k + 2 < n; k++) {
        if (!((surviveMask >> k) & 1u)) continue;
        Record rec{};
        uint32_t rect = 0;
        setupSubTriangle(polyA, k, tid, p.width, p.height, &rec.s, &rect);
        rec.t = t;
        if (slot < p.capacity) { // (always: at most 6 per triangle and the launcher sized the arrays for that many)
            p.rects[slot] = rect;
            p.records[slot] = rec;
        }
        slot++;
    }
}

struct TextureInputs {
    static constexpr bool kFormats = false, kAniso = false;
    const float* uvs; const Material* materials; const Texture* textures; const uint32_t* texels;
    uint64_t uvVertexCount, texelCount;
    uint32_t drawCount, textureCount;
};
// a format-aware execution's (textureFormats = 1): one format code per texture; texelCount counts the uint32 words of `texels`. The other instantiations keep
// TextureInputs, and with it their argument blocks and their LDS
struct FormatTextureInputs : TextureInputs {
    static constexpr bool kFormats = true;
    const uint32_t* formats;
};
// an anisotropic execution's (maxAnisotropy 2 .. 16): always format-aware - `formats` is null where textureFormats is 0, and every texture is RGBA8 then
struct AnisoTextureInputs : FormatTextureInputs {
    static constexpr bool kAniso = true;
    uint32_t maxAnisotropy;
};
template <bool kFormats, bool kAniso = false> struct TextureInputsOf { typedef TextureInputs type; };
template <> struct TextureInputsOf<true, false> { typedef FormatTextureInputs type; };
template <> struct TextureInputsOf<true, true> { typedef AnisoTextureInputs type; };
// A of the anisotropic contract; 0 in every other instantiation, which never reads it
template <class Tex> PLR_DI uint32_t maxAnisotropyOf(const Tex& tex) {
    if constexpr (Tex::kAniso) return tex.maxAnisotropy;
    else return 0u;
}
struct TileParams {
    ScratchHeader* header; const TriangleOrigin* origins; const uint32_t* rects; const Record* records;
    const float* transforms; const float* positions; const float* normals; const uint32_t* indices; const Draw* draws;
    const GlobalUbo* global;
    float* depth; uint32_t* motion; uint32_t* normal; uint32_t* albedo; uint32_t* specular;
    uint32_t capacity, triangleCount;
    int32_t width, height;
    int32_t windowTileX0, windowTileY0; // the window's first tile: the grid is the window's tiles (0, 0 without a window)
    TextureInputs tex; // a textured execution only (behind everything else: the untextured kernel's argument offsets stay)
    const uint32_t* alphaCutoffs; // an alpha-tested execution only: tex.drawCount words
};
// a normal-mapped execution's tile kernel leaves the winner's t in the shadingNormal texel (the other instantiations keep their argument block)
struct NormalTileParams : TileParams { uint32_t* shadingNormal; };
template <bool kNormalMap, bool kFormats = false, bool kAniso = false> struct TileParamsOf { typedef TileParams type; };
template <> struct TileParamsOf<true, false, false> { typedef NormalTileParams type; };
// a format-aware execution's: binding 14 behind everything else
struct FormatTileParams : TileParams { const uint32_t* formats; };
struct FormatNormalTileParams : NormalTileParams { const uint32_t* formats; };
template <> struct TileParamsOf<false, true, false> { typedef FormatTileParams type; };
template <> struct TileParamsOf<true, true, false> { typedef FormatNormalTileParams type; };
// an anisotropic execution's: the seventh push-constant word behind everything else
struct AnisoTileParams : FormatTileParams { uint32_t maxAnisotropy; };
struct AnisoNormalTileParams : FormatNormalTileParams { uint32_t maxAnisotropy; };
template <> struct TileParamsOf<false, true, true> { typedef AnisoTileParams type; };
template <> struct TileParamsOf<true, true, true> { typedef AnisoNormalTileParams type; };

typedef unsigned long long Key;

PLR_DI void keepFragment(float zf, uint32_t t, Key* cell) {
    if (!(zf > 0.f)) return; // at or beyond the far plane, or a NaN
    atomicMax(cell, ((Key)f2u(zf) << 32) | (Key)t);
}

struct D3 { double x, y, z; };
PLR_DI double det3(D3 a, D3 b, D3 c) { return (a.x * (b.y * c.z - b.z * c.y) - a.y * (b.x * c.z - b.z * c.x)) + a.z * (b.x * c.y - b.y * c.x); }
PLR_DI double weighted(const double b[3], double a0, double a1, double a2) { return (b[0] * a0 + b[1] * a1) + b[2] * a2; }
PLR_DI D3 normalized(D3 v) {
    const double len = __builtin_sqrt((v.x * v.x + v.y * v.y) + v.z * v.z);
    if (!(len > 0.0 && len < __builtin_inf())) return D3{0.0, 0.0, 0.0};
    return D3{v.x / len, v.y / len, v.z / len};
}
PLR_DI uint32_t snorm16(float m) {
    if (m != m) return 0u;
    return (uint32_t)(int32_t)__builtin_rintf(fminf(fmaxf(m, -1.f), 1.f) * 32767.f) & 0xffffu;
}
PLR_DI uint32_t unorm8Half(float n) { // n * 0.5 + 0.5 under the image contract's UNORM8 rule
    const float v = n * 0.5f + 0.5f;
    if (v != v) return 0u;
    return (uint32_t)(int32_t)__builtin_rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f);
}

// ---- material textures (the sampling contract)
// b of a triangle with the clip (x, y, w) V_k at the point P; s zero or non-finite: (1, 0, 0)
PLR_DI void barycentricsAt(D3 P, const D3 V[3], double b[3]) {
    const double e0 = det3(P, V[1], V[2]), e1 = det3(P, V[2], V[0]), e2 = det3(P, V[0], V[1]);
    const double s = (e0 + e1) + e2;
    b[0] = 1.0; b[1] = 0.0; b[2] = 0.0;
    if (s != 0.0 && __builtin_fabs(s) < __builtin_inf()) { b[0] = e0 / s; b[1] = e1 / s; b[2] = e2 / s; }
}

// t mod n in [0, n) for |t| < 2^35 and 1 <= n <= 2^14: t / n is an integer or at least 2^-14 away from one, 16 times the spacing of fp64 at 2^34, so the floor
// of the fp64 quotient is the exact one (a 64-bit integer division costs an order of magnitude more instructions)
PLR_DI int wrapRepeat(int64_t t, int n) {
    const double q = __builtin_floor((double)t / (double)n);
    return (int)(t - (int64_t)q * (int64_t)n);
}

struct TexelSums { uint32_t c[4]; }; // per channel: 16 bits of weight on 8 bits of code

// ---- block-compressed textures (the block decode contract). A format-aware instantiation carries a usable texture's format code in bits 16 - 31 of the
// Texture's mipCount (usableTexture puts it there; a usable mipCount is at most 15), so that an AlphaRecord keeps its 36 words
template <bool kFormats> PLR_DI uint32_t mipCountOf(const Texture& t) { return kFormats ? t.mipCount & 0xffffu : t.mipCount; }
template <bool kFormats> PLR_DI uint32_t formatOf(const Texture& t) { return kFormats ? t.mipCount >> 16 : kTextureFormatRgba8; }
// the uint32 words of a w x h level of `format`
PLR_DI uint64_t levelWords(uint32_t format, uint32_t w, uint32_t h) {
    if (format != kTextureFormatRgba8) return (uint64_t)((w + 3u) >> 2) * (uint64_t)((h + 3u) >> 2) * (format == kTextureFormatBc1 ? 2u : 4u);
    return (uint64_t)w * (uint64_t)h;
}
// colourBlockTexel, alphaBlockTexel and blockTexel - the decode of one texel of a block - live in device/bc_decode.h: "sceneMeanAlbedo.comp" reads the same blocks

// the four taps of one level (dimensions w x h, first texel at `base`), weighted; every address in 64 bits and checked against texelCount before its load
template <int kFirst = 0, bool kFormats = false>
PLR_DI TexelSums bilinearTaps(const uint32_t* texels, uint64_t texelCount, uint64_t base, int w, int h, double u, double v, uint32_t format = kTextureFormatRgba8) {
    const int64_t Tu = (int64_t)__builtin_floor((u * (double)w - 0.5) * 256.0 + 0.5), Tv = (int64_t)__builtin_floor((v * (double)h - 0.5) * 256.0 + 0.5);
    const uint32_t fx = (uint32_t)(Tu & 255), fy = (uint32_t)(Tv & 255);
    const int x0 = wrapRepeat(Tu >> 8, w), y0 = wrapRepeat(Tv >> 8, h);
    const int x1 = x0 + 1 == w ? 0 : x0 + 1, y1 = y0 + 1 == h ? 0 : y0 + 1;
    auto fetch = [&](int x, int y) {
        if constexpr (kFormats) {
            if (format != kTextureFormatRgba8) return blockTexel<kFirst>(texels, texelCount, base, format, w, x, y);
        }
        const uint64_t at = base + (uint64_t)y * (uint64_t)w + (uint64_t)x;
        return at < texelCount ? texels[at] : 0u;
    };
    const uint32_t c00 = fetch(x0, y0), c10 = fetch(x1, y0), c01 = fetch(x0, y1), c11 = fetch(x1, y1);
    const uint32_t w00 = (256u - fx) * (256u - fy), w10 = fx * (256u - fy), w01 = (256u - fx) * fy, w11 = fx * fy;
    TexelSums out;
    for (int k = kFirst; k < 4; k++)
        out.c[k] = w00 * ((c00 >> (8 * k)) & 255u) + w10 * ((c10 >> (8 * k)) & 255u) + w01 * ((c01 >> (8 * k)) & 255u) + w11 * ((c11 >> (8 * k)) & 255u);
    return out;
}

// one trilinear sample of `texture`: (u, v) for the taps, (dudx, dvdx) and (dudy, dvdy) the raw forward differences. kFirst: the first channel computed - 3 is
// the alpha-only sample of the coverage path, whose bits 24 - 31 are those of the full word because every channel is filtered by itself
// kAniso (the anisotropic contract): (u, v) are the RAW ones, the validity rule is applied per probe here; maxAniso is A, 2 .. 16
template <int kFirst = 0, bool kFormats = false, bool kAniso = false>
PLR_DI uint32_t sampleTexture(const TextureInputs& tex, Texture texture, double u, double v, double dudx, double dvdx, double dudy, double dvdy, float mipBias,
                              uint32_t maxAniso = 0u) {
    const double w0 = (double)texture.width, h0 = (double)texture.height;
    const double axx = dudx * w0, axy = dvdx * h0, ayx = dudy * w0, ayy = dvdy * h0;
    const double rx = axx * axx + axy * axy, ry = ayx * ayx + ayy * ayy;
    const double rho2 = rx > ry ? rx : ry;
    float r = (float)rho2;
    uint32_t probes = 1u; // N
    if constexpr (kAniso) {
        const double rmin = rx > ry ? ry : rx;
        // the contract's loop stops at the first n with !(n n rmin < rmax); rmin >= 0 or a NaN, so n n rmin does not decrease with n and the test, once false, stays
        // false: N = 1 + the number of n in [1, A) that pass. A is wave-uniform: this loop has a scalar trip count and no exec mask (a NaN passes none: N = 1)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
        for (uint32_t n = 1u; n < maxAniso; n++) probes += (double)(n * n) * rmin < rho2 ? 1u : 0u;
        r = (float)(rho2 / (double)(probes * probes));
    }
    float lod = 0.5f * det_log2f(r) + mipBias;
    if (!(lod > 0.f)) lod = 0.f;
    const uint32_t mipCount = mipCountOf<kFormats>(texture), format = formatOf<kFormats>(texture);
    const float top = (float)(mipCount - 1u);
    if (lod > top) lod = top;
    const int q = (int)__builtin_floorf(lod * 256.f + 0.5f);
    const int L0 = q >> 8, L1 = min(L0 + 1, (int)mipCount - 1);
    const uint32_t fw = (uint32_t)(q & 255);
    uint64_t base = texture.texelOffset;
    for (int l = 0; l < L0; l++) {
        if constexpr (kFormats) base += levelWords(format, max(1u, texture.width >> l), max(1u, texture.height >> l));
        else base += (uint64_t)max(1u, texture.width >> l) * (uint64_t)max(1u, texture.height >> l);
    }
    const int w = (int)max(1u, texture.width >> L0), h = (int)max(1u, texture.height >> L0);
    if constexpr (kAniso) {
        // N probes along the major axis at the shared L0, L1, fw; T = the sum of their trilinear integer sums, the code T / (N 2^24) rounded half to even. The
        // loop stays rolled and runs to this lane's own N
        const bool majorX = rx > ry;
        // N = 1: the one probe is (u, v) with no arithmetic on it. Its t is 0, and with (du, dv) = (0, 0) for such a lane u + 0 * 0 is u, value for value (a NaN
        // stays one, -0 becomes +0, which no tap tells apart) - without a per-lane condition held across the loop
        const double du = probes == 1u ? 0.0 : majorX ? dudx : dudy, dv = probes == 1u ? 0.0 : majorX ? dvdx : dvdy;
        uint64_t base1 = base;
        if (L1 != L0) base1 += levelWords(format, (uint32_t)w, (uint32_t)h);
        const int w1 = (int)max(1u, texture.width >> L1), h1 = (int)max(1u, texture.height >> L1);
        uint64_t T[4] = {0ull, 0ull, 0ull, 0ull};
        // one step per (probe, level): a single copy of the taps serves both levels, and L1's steps do not exist where fw == 0
        const uint32_t twoLevels = fw != 0u ? 1u : 0u, steps = probes << twoLevels;
        // a lane runs to its own N; the loop's exit is the wave's (a ballot and a scalar branch: one exec mask held, not a divergent loop's two), and the lane
        // counts its own steps down, so that the step's small integers live in vector registers: the alpha-tested scan has no scalar register to spare
#pragma unroll 1
        for (uint32_t left = steps; __ballot(left != 0u) != 0ull;) {
            if (left == 0u) continue;
            const uint32_t i = steps - left;
            left--;
            const uint32_t k = i >> twoLevels;
            const bool upper = (i & twoLevels) != 0u;
            const double t = (double)(2 * (int)k + 1 - (int)probes) / (double)(2u * probes);
            double pu = u + t * du, pv = v + t * dv;
            if (!(__builtin_fabs(pu) < 1048576.0 && __builtin_fabs(pv) < 1048576.0)) pu = pv = 0.0; // the validity rule, per probe (a NaN fails the comparison)
            const TexelSums s = bilinearTaps<kFirst, true>(tex.texels, tex.texelCount, upper ? base1 : base, upper ? w1 : w, upper ? h1 : h, pu, pv, format);
            const uint32_t weight = upper ? fw : 256u - fw; // weight * s.c <= 256 * 255 * 2^16: fits uint32
            for (int c = kFirst; c < 4; c++) T[c] += (uint64_t)(weight * s.c[c]);
        }
        // qd = floor(T / D), D = N 2^24: floor((T >> 24) / N) is the same integer; T >> 24 < 2^12 and N <= 16 are exact in fp32, and their quotient is an integer or
        // at least 1 / 16 away from one, 2^7 times the spacing of fp32 below 2^12: the truncated, correctly rounded fp32 quotient is the exact one
        const uint64_t D = (uint64_t)probes << 24;
        const float fn = (float)probes;
        uint32_t word = 0u;
        for (int c = kFirst; c < 4; c++) {
            const uint32_t qd = (uint32_t)((float)(uint32_t)(T[c] >> 24) / fn);
            const uint64_t twice = 2ull * (T[c] - (uint64_t)qd * D);
            word |= (qd + (uint32_t)(twice > D || (twice == D && (qd & 1u)))) << (8 * c);
        }
        return word;
    }
    const TexelSums s0 = bilinearTaps<kFirst, kFormats>(tex.texels, tex.texelCount, base, w, h, u, v, format);
    TexelSums s1{{0u, 0u, 0u, 0u}};
    if (fw != 0u) { // (with fw == 0 the upper level has no weight; with L1 == L0 it is the same level again)
        uint64_t base1 = base;
        if constexpr (kFormats) base1 += L1 == L0 ? 0u : levelWords(format, (uint32_t)w, (uint32_t)h);
        else base1 = L1 == L0 ? base : base + (uint64_t)w * (uint64_t)h;
        s1 = bilinearTaps<kFirst, kFormats>(tex.texels, tex.texelCount, base1, (int)max(1u, texture.width >> L1), (int)max(1u, texture.height >> L1), u, v, format);
    }
    uint32_t word = 0u;
    for (int k = kFirst; k < 4; k++) {
        const uint32_t S = (256u - fw) * s0.c[k] + fw * s1.c[k];
        word |= ((S + 0x7fffffu + ((S >> 24) & 1u)) >> 24) << (8 * k);
    }
    return word;
}

// the table entry `index` names when it is usable: inside the table, 1 <= width, height <= 16384, 1 <= mipCount <= floor(log2(max(width, height))) + 1
// A format-aware execution (Tex::kFormats): also a format code of at most 3 and, for a compressed entry, a texelOffset that is a multiple of its block's words;
// the format code goes into bits 16 - 31 of out->mipCount (mipCountOf, formatOf)
template <class Tex>
PLR_DI bool usableTexture(const Tex& tex, uint32_t index, Texture* out) {
    if (index == kNoTexture || index >= tex.textureCount) return false;
    const Texture t = tex.textures[index];
    if (t.width < 1u || t.height < 1u || t.width > kMaxTextureSize || t.height > kMaxTextureSize) return false;
    if (t.mipCount < 1u || t.mipCount > 32u - (uint32_t)__clz(max(t.width, t.height))) return false;
    *out = t;
    if constexpr (Tex::kFormats) {
        uint32_t format;
        if constexpr (Tex::kAniso) format = tex.formats ? tex.formats[index] : kTextureFormatRgba8; // (wave-uniform: no binding 14, every texture is RGBA8)
        else format = tex.formats[index];
        if (format > kTextureFormatBc5) return false;
        if (format != kTextureFormatRgba8 && (t.texelOffset & (format == kTextureFormatBc1 ? 1u : 3u)) != 0u) return false;
        out->mipCount = t.mipCount | (format << 16);
    }
    return true;
}

// V_k, the UV fetch and the sample point of the resolve and of the alpha test: one text, so a fragment's alpha is the alpha the resolve stores
PLR_DI D3 clipXYW(const float* M, const float* q) {
    return D3{(double)clipComponent(M, 0, q[0], q[1], q[2]), (double)clipComponent(M, 1, q[0], q[1], q[2]), (double)clipComponent(M, 3, q[0], q[1], q[2])};
}
PLR_DI void fetchUv(const TextureInputs& tex, uint64_t vertex, double* u, double* v) { // a vertex outside `uvs` has (0, 0)
    const bool inside = vertex < tex.uvVertexCount;
    *u = inside ? (double)tex.uvs[vertex * 2u] : 0.0;
    *v = inside ? (double)tex.uvs[vertex * 2u + 1u] : 0.0;
}
struct UvSample { double u, v, dudx, dvdx, dudy, dvdy; }; // (u, v) validated for the taps, the forward differences raw
// kRaw (an anisotropic execution): (u, v) stay raw - sampleTexture<., ., true> validates every probe itself
template <bool kRaw = false>
PLR_DI UvSample uvSampleAt(D3 P, const double b[3], const D3 V[3], const double tu[3], const double tv[3], int x, int y, int width, int height) {
    double bx[3], by[3];
    barycentricsAt(D3{(double)(2 * (x + 1) + 1) / (double)width - 1.0, P.y, 1.0}, V, bx);
    barycentricsAt(D3{P.x, (double)(2 * (y + 1) + 1) / (double)height - 1.0, 1.0}, V, by);
    UvSample s;
    s.u = weighted(b, tu[0], tu[1], tu[2]); s.v = weighted(b, tv[0], tv[1], tv[2]);
    s.dudx = weighted(bx, tu[0], tu[1], tu[2]) - s.u; s.dvdx = weighted(bx, tv[0], tv[1], tv[2]) - s.v;
    s.dudy = weighted(by, tu[0], tu[1], tu[2]) - s.u; s.dvdy = weighted(by, tv[0], tv[1], tv[2]) - s.v;
    if constexpr (!kRaw) {
        if (!(__builtin_fabs(s.u) < 1048576.0 && __builtin_fabs(s.v) < 1048576.0)) s.u = s.v = 0.0; // (a NaN fails the comparison)
    }
    return s;
}

// the winner's vertex fetch, mat3(model) * v and N_k: one text for the resolve and for the shading-normal kernel, so the vertex normal the latter interpolates is
// the one behind `normal`. The vertices are inside `positions` and `normals`: the set-up kernel made a record of this triangle
PLR_DI void fetchWinnerVertices(const uint32_t* indices, const float* positions, const float* normals, uint64_t at, uint32_t vertexOffset, uint64_t vertex[3], float pos[3][3],
                                float nrm[3][3]) {
    for (int k = 0; k < 3; k++) {
        const uint64_t v = (uint64_t)indices[at + k] + (uint64_t)vertexOffset;
        vertex[k] = v;
        for (int c = 0; c < 3; c++) { pos[k][c] = positions[v * 3u + c]; nrm[k][c] = normals[v * 3u + c]; }
    }
}
PLR_DI D3 rotated(const float* model, D3 in) { // mat3(model) * in: component r = (m[0][r] x + m[1][r] y) + m[2][r] z
    return D3{((double)model[0] * in.x + (double)model[4] * in.y) + (double)model[8] * in.z, ((double)model[1] * in.x + (double)model[5] * in.y) + (double)model[9] * in.z,
              ((double)model[2] * in.x + (double)model[6] * in.y) + (double)model[10] * in.z};
}
PLR_DI void vertexNormals(const float pos[3][3], const float nrm[3][3], const float* model, D3 N[3]) {
    D3 face{0.0, 0.0, 0.0};
    {
        const D3 a{(double)pos[0][0] - (double)pos[2][0], (double)pos[0][1] - (double)pos[2][1], (double)pos[0][2] - (double)pos[2][2]};
        const D3 c{(double)pos[0][0] - (double)pos[1][0], (double)pos[0][1] - (double)pos[1][1], (double)pos[0][2] - (double)pos[1][2]};
        face = normalized(D3{a.y * c.z - a.z * c.y, a.z * c.x - a.x * c.z, a.x * c.y - a.y * c.x});
    }
    for (int k = 0; k < 3; k++) {
        D3 in{(double)nrm[k][0], (double)nrm[k][1], (double)nrm[k][2]};
        if (nrm[k][0] == 0.f && nrm[k][1] == 0.f && nrm[k][2] == 0.f) in = face;
        N[k] = normalized(rotated(model, in));
    }
}

// the winner's attributes at pixel (x, y): motion, normal and the draw's two material words (kTextured: the sampled texel where its material names a texture)
template <bool kTextured, class Tex>
PLR_DI void resolvePixel(const TileParams& p, const Tex& tex, uint32_t t, int x, int y, uint32_t* motion, uint32_t* normal, uint32_t* albedo, uint32_t* specular) {
    const TriangleOrigin o = p.origins[t];
    const Draw draw = p.draws[o.draw];
    const uint64_t at = (uint64_t)draw.firstIndex + (uint64_t)o.local * 3u;
    const float* T = p.transforms + (size_t)draw.transformIndex * 48u;
    const float *model = T, *mvp = T + 16, *mvpPrevious = T + 32;
    float pos[3][3], nrm[3][3];
    D3 V[3], prev[3];
    uint64_t vertex[3];
    fetchWinnerVertices(p.indices, p.positions, p.normals, at, draw.vertexOffset, vertex, pos, nrm);
    for (int k = 0; k < 3; k++) {
        V[k] = clipXYW(mvp, pos[k]);
        prev[k] = clipXYW(mvpPrevious, pos[k]);
    }
    const D3 P{(double)(2 * x + 1) / (double)p.width - 1.0, (double)(2 * y + 1) / (double)p.height - 1.0, 1.0};
    double b[3];
    barycentricsAt(P, V, b);
    // normal
    D3 N[3];
    vertexNormals(pos, nrm, model, N);
    const D3 nn = normalized(D3{weighted(b, N[0].x, N[1].x, N[2].x), weighted(b, N[0].y, N[1].y, N[2].y), weighted(b, N[0].z, N[1].z, N[2].z)});
    *normal = unorm8Half((float)nn.x) | (unorm8Half((float)nn.y) << 8) | (unorm8Half((float)nn.z) << 16) | (255u << 24);
    // motion
    const double ws = weighted(b, prev[0].z, prev[1].z, prev[2].z);
    uint32_t code = 0u;
    if (ws > 0.0 && ws < __builtin_inf()) {
        const double xs = weighted(b, prev[0].x, prev[1].x, prev[2].x), ys = weighted(b, prev[0].y, prev[1].y, prev[2].y);
        const double px = xs / ws + (double)p.global->previousFrameCameraJitter[0], py = ys / ws + (double)p.global->previousFrameCameraJitter[1];
        const double cx = P.x + (double)p.global->currentFrameCameraJitter[0], cy = P.y + (double)p.global->currentFrameCameraJitter[1];
        code = snorm16((float)((px - cx) * 0.5)) | (snorm16((float)((py - cy) * 0.5)) << 16);
    }
    *motion = code;
    *albedo = draw.albedo;
    *specular = draw.specular;
    if constexpr (kTextured) {
        if (o.draw >= tex.drawCount) return;
        const Material material = tex.materials[o.draw];
        Texture albedoTexture, specularTexture;
        const bool sampleAlbedo = usableTexture(tex, material.albedoTexture, &albedoTexture), sampleSpecular = usableTexture(tex, material.specularTexture, &specularTexture);
        if (!sampleAlbedo && !sampleSpecular) return;
        double tu[3], tv[3];
        for (int k = 0; k < 3; k++) fetchUv(tex, vertex[k], &tu[k], &tv[k]);
        const UvSample uv = uvSampleAt<Tex::kAniso>(P, b, V, tu, tv, x, y, p.width, p.height);
        const float mipBias = p.global->mipBias;
        const uint32_t maxAniso = maxAnisotropyOf(tex);
        if (sampleAlbedo) *albedo = sampleTexture<0, Tex::kFormats, Tex::kAniso>(tex, albedoTexture, uv.u, uv.v, uv.dudx, uv.dvdx, uv.dudy, uv.dvdy, mipBias, maxAniso);
        if (sampleSpecular) *specular = sampleTexture<0, Tex::kFormats, Tex::kAniso>(tex, specularTexture, uv.u, uv.v, uv.dudx, uv.dvdx, uv.dudy, uv.dvdy, mipBias, maxAniso);
    }
}

// ---- the alpha test (the alpha test contract)
// what the fragments of one record need, found once per record through origins[t].draw -> alphaCutoffs[draw]
struct AlphaRecord {
    uint32_t cutoff; // kAlphaCutoffOpaque: every fragment passes (an opaque draw, or a constant alpha >= c); kAlphaCutoffDiscardAll: none does; else the sample decides
    Texture texture; // } of a sampled record only
    uint32_t t;      // }
    D3 V[3];         // }
    double tu[3], tv[3];
};
constexpr uint32_t kAlphaRecordWords = 36;
static_assert(sizeof(AlphaRecord) == kAlphaRecordWords * 4, "AlphaRecord is moved through LDS word by word");
PLR_DI bool alphaSampled(uint32_t cutoff) { return cutoff != kAlphaCutoffOpaque && cutoff != kAlphaCutoffDiscardAll; }
struct AlphaInputs { const uint32_t* cutoffs; float mipBias; };

template <class Tex>
PLR_DI void alphaOfRecord(const TileParams& p, const Tex& tex, const uint32_t* cutoffs, uint32_t t, AlphaRecord& a) {
    a.cutoff = kAlphaCutoffOpaque;
    if (t >= p.triangleCount) return; // (never: the set-up kernel wrote t)
    const TriangleOrigin o = p.origins[t];
    if (o.draw >= tex.drawCount) return; // (never: cutoffs, materials and draws hold drawCount entries)
    const uint32_t c = min(cutoffs[o.draw], kAlphaCutoffDiscardAll);
    if (c == kAlphaCutoffOpaque || c == kAlphaCutoffDiscardAll) { a.cutoff = c; return; }
    const Draw draw = p.draws[o.draw];
    if (!usableTexture(tex, tex.materials[o.draw].albedoTexture, &a.texture)) { // the draw's constant word decides for all its fragments
        a.cutoff = (draw.albedo >> 24) >= c ? kAlphaCutoffOpaque : kAlphaCutoffDiscardAll;
        return;
    }
    // the vertices are inside their buffers: the set-up kernel made a record of this triangle (resolvePixel relies on the same)
    const uint64_t at = (uint64_t)draw.firstIndex + (uint64_t)o.local * 3u;
    const float* mvp = p.transforms + (size_t)draw.transformIndex * 48u + 16u;
    uint64_t vertex[3];
    for (int k = 0; k < 3; k++) {
        vertex[k] = (uint64_t)p.indices[at + k] + (uint64_t)draw.vertexOffset;
        float pos[3];
        for (int c3 = 0; c3 < 3; c3++) pos[c3] = p.positions[vertex[k] * 3u + c3];
        a.V[k] = clipXYW(mvp, pos);
    }
    for (int k = 0; k < 3; k++) fetchUv(tex, vertex[k], &a.tu[k], &a.tv[k]);
    a.cutoff = c;
    a.t = t;
}

// a(t, i, j): bits 24 - 31 of the albedo word the resolve would store for this triangle at pixel (x, y) - the same functions in the same order
template <bool kFormats, bool kAniso = false>
PLR_DI uint32_t fragmentAlpha(const TextureInputs& tex, const AlphaRecord& a, float mipBias, int x, int y, int width, int height, uint32_t maxAniso = 0u) {
    const D3 P{(double)(2 * x + 1) / (double)width - 1.0, (double)(2 * y + 1) / (double)height - 1.0, 1.0};
    double b[3];
    barycentricsAt(P, a.V, b);
    const UvSample uv = uvSampleAt<kAniso>(P, b, a.V, a.tu, a.tv, x, y, width, height);
    return sampleTexture<3, kFormats, kAniso>(tex, a.texture, uv.u, uv.v, uv.dudx, uv.dvdx, uv.dudy, uv.dvdy, mipBias, maxAniso) >> 24;
}

// THE ALPHA-TESTED SCAN. A sample costs far more than coverage, a stamp of a triangle's box or a lane's 4 x 4 box is seldom full, and the loads that lead to a
// record's vertices depend on one another. So per step of 64 records every lane finds the alpha data of ITS record at once (one chain of loads per step, not
// per record) and leaves it in LDS (`records`: word-major, a column per lane); the lane path and the wave path then only QUEUE their candidates - fragments that
// passed coverage, zf > 0 and the early out - with the slot of their record (in LDS, `queue`), and the wave samples 64 candidates at a time, one per lane, and
// what is left at the end of the step.
struct Candidate { uint32_t xy; float zf; uint32_t slot; }; // x | y << 16 (the frame is at most 16384 wide and high); slot: the lane that holds the record
constexpr uint32_t kCandidateSlots = 128;                   // fewer than 64 pending + at most 64 of one push

template <class Tex> struct AlphaScan {
    Candidate* queue;                 // this wave's kCandidateSlots entries
    uint32_t (*records)[64];          // this wave's kAlphaRecordWords x 64 words
    const Tex* tex;
    float mipBias;
    int width, height;
    Key* tile;
    int ox, oy;
    uint32_t lane;
    uint32_t pending;                 // (wave-uniform)

    PLR_DI void store(const AlphaRecord& a) {
        union { AlphaRecord r; uint32_t w[kAlphaRecordWords]; } u;
        u.r = a;
        for (uint32_t k = 0; k < kAlphaRecordWords; k++) records[k][lane] = u.w[k];
    }
    // A fragment whose key is not above its cell is dropped before the sample: the result is a maximum, so the image is the same (the plain read is a filter,
    // the atomic decides)
    PLR_DI void sample(uint32_t count) {
        if (lane < count) {
            const uint32_t xy = queue[lane].xy, slot = queue[lane].slot;
            const float zf = queue[lane].zf;
            union { AlphaRecord r; uint32_t w[kAlphaRecordWords]; } u;
            for (uint32_t k = 0; k < kAlphaRecordWords; k++) u.w[k] = records[k][slot];
            const int px = (int)(xy & 0xffffu), py = (int)(xy >> 16);
            Key* cell = &tile[(py - oy) * kTileSize + (px - ox)];
            const Key key = ((Key)f2u(zf) << 32) | (Key)u.r.t;
            if (key > *cell && fragmentAlpha<Tex::kFormats, Tex::kAniso>(*tex, u.r, mipBias, px, py, width, height, maxAnisotropyOf(*tex)) >= u.r.cutoff) atomicMax(cell, key);
        }
    }
    // called by the whole wave: the lanes with `candidate` append theirs; a full wave of candidates is sampled at once
    PLR_DI void push(bool candidate, int px, int py, float zf, uint32_t slot) {
        const unsigned long long mask = __ballot(candidate);
        if (mask == 0ull) return;
        if (candidate) {
            Candidate& c = queue[pending + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))];
            c.xy = (uint32_t)px | ((uint32_t)py << 16); c.zf = zf; c.slot = slot;
        }
        pending += (uint32_t)__popcll(mask);
        __builtin_amdgcn_wave_barrier(); // (one wave: its LDS operations execute in order)
        if (pending >= 64u) {
            sample(64u);
            pending -= 64u;
            uint32_t xy = 0u, slot = 0u;
            float zf = 0.f;
            if (lane < pending) { xy = queue[64u + lane].xy; zf = queue[64u + lane].zf; slot = queue[64u + lane].slot; }
            __builtin_amdgcn_wave_barrier();
            if (lane < pending) { queue[lane].xy = xy; queue[lane].zf = zf; queue[lane].slot = slot; }
            __builtin_amdgcn_wave_barrier();
        }
    }
    PLR_DI void flush() {
        sample(pending);
        pending = 0u;
        __builtin_amdgcn_wave_barrier();
    }
    // is a covered fragment of triangle t with depth zf at (px, py) a candidate: kept by the zf > 0 rule and above its cell (the early out)?
    PLR_DI bool above(uint32_t t, int px, int py, float zf) const { return zf > 0.f && (((Key)f2u(zf) << 32) | (Key)t) > tile[(py - oy) * kTileSize + (px - ox)]; }
};

// what becomes of a fragment without the alpha test: the pixel's key, by 64-bit maximum. tile: the block's 64 x 64 keys, (ox, oy) its first pixel
struct KeyWalk : rastercov::PlainWalk {
    Key* tile;
    int ox, oy;
    static PLR_DI const SetupRecord& setup(const Record& r) { return r.s; }
    template <class D> PLR_DI void fragment(const Record& r, int, int px, int py, D&& depthAt) {
        float zf;
        if (depthAt(&zf)) keepFragment(zf, r.t, &tile[(py - oy) * kTileSize + (px - ox)]);
    }
};

// ... and with the alpha test, through all the hooks of rastercov::rasteriseTile: a fragment of an opaque draw's record goes KeyWalk's way, one of a discarded
// draw's nowhere, and the candidates of a sampled record go into AlphaScan's queue
template <class Tex> struct AlphaWalk {
    AlphaScan<Tex> scan;
    const TileParams* q;
    const AlphaInputs* inputs;
    uint32_t myCutoff;    // of this lane's record
    uint32_t stampCutoff; // (wave-uniform) of the record the wave stamps; opaque outside the stamp path

    static PLR_DI const SetupRecord& setup(const Record& r) { return r.s; }
    // every lane's record at once: its draw's cutoff and, where the sample decides, its texture, V_k and UVs. Then the lane path of the sampled records: the <= 16
    // pixels of every lane's box in step, so that the candidates can be queued
    PLR_DI void beginStep(const Record& rr, bool hit, bool small, int bx0, int by0, int bx1, int by1) {
        scan.mipBias = inputs->mipBias; scan.width = q->width; scan.height = q->height;
        myCutoff = stampCutoff = kAlphaCutoffOpaque;
        if (hit) {
            AlphaRecord a;
            alphaOfRecord(*q, *scan.tex, inputs->cutoffs, rr.t, a);
            myCutoff = a.cutoff;
            if (alphaSampled(a.cutoff)) scan.store(a);
        }
        __builtin_amdgcn_wave_barrier();
        const bool laneTested = small && alphaSampled(myCutoff);
        if (__ballot(laneTested)) {
            const EdgeSteps steps(rr.s); // (fa: a narrow record's area fits int32, so the int64 conversion gives the int32 one's value)
            for (int o = 0; o < 16; o++) {
                const int px = bx0 + (o & 3), py = by0 + (o >> 2);
                float zf = 0.f;
                const bool candidate = laneTested && px <= bx1 && py <= by1 &&
                                       ((rr.s.topLeft & kNarrowFlag) ? rastercov::fragmentDepthNarrow(rr.s, steps.fa, px, py, &zf) : rastercov::fragmentDepth(rr.s, steps, px, py, &zf)) &&
                                       scan.above(rr.t, px, py, zf);
                scan.push(candidate, px, py, zf, scan.lane);
            }
        }
    }
    PLR_DI bool lanePath() const { return myCutoff == kAlphaCutoffOpaque; }
    PLR_DI bool beginStamps(int src) {
        stampCutoff = (uint32_t)__builtin_amdgcn_readlane((int)myCutoff, src);
        return stampCutoff != kAlphaCutoffDiscardAll;
    }
    // the stamps of a sampled record queue their candidates with the slot of the record's lane (the whole wave calls)
    template <class D> PLR_DI void fragment(const Record& r, int slot, int px, int py, D&& depthAt) {
        float zf = 0.f;
        if (stampCutoff == kAlphaCutoffOpaque) {
            if (depthAt(&zf)) keepFragment(zf, r.t, &scan.tile[(py - scan.oy) * kTileSize + (px - scan.ox)]);
        } else
            scan.push(depthAt(&zf) && scan.above(r.t, px, py, zf), px, py, zf, (uint32_t)slot);
    }
    PLR_DI void endStep() { scan.flush(); } // before the next step's records replace these
};

// kNormalMap: the resolve also leaves the winner's t (kNoWinner: none) in the shadingNormal texel, for depthPrepassShadingNormalKernel behind this kernel
// kFormats: the format-aware instantiations (textureFormats = 1) - the same text with the block decode behind every tap
// kAniso: the anisotropic instantiations (maxAnisotropy 2 .. 16) - format-aware all of them, with the probe loop behind every sample
template <bool kTextured, bool kAlphaTest = false, bool kNormalMap = false, bool kFormats = false, bool kAniso = false>
__global__ __launch_bounds__(256) void depthPrepassTileKernel(typename TileParamsOf<kNormalMap, kFormats, kAniso>::type p) {
    typedef typename TileParamsOf<kNormalMap, kFormats, kAniso>::type Params;
    typedef typename TextureInputsOf<kFormats, kAniso>::type Tex;
    static_assert(kFormats || !kAniso, "the anisotropic instantiations exist in the format-aware form only");
    static_assert(kTextured || !kFormats, "a format belongs to a texture");
    static_assert(kTextured || !kAlphaTest, "the alpha of a fragment is a texture sample");
    static_assert(kTextured || !kNormalMap, "the shading normal is a texture sample");
    __shared__ Key tile[kTileSize * kTileSize];
    __shared__ uint32_t hitQueue[4][256]; // per wave: the entries of the current step that touch the tile
    const int tx = (int)blockIdx.x + p.windowTileX0, ty = (int)blockIdx.y + p.windowTileY0;
    const int ox = tx * kTileSize, oy = ty * kTileSize;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < (uint32_t)(kTileSize * kTileSize); i += 256u) tile[i] = 0ull;
    // the textured resolve takes its inputs from LDS: held in scalar registers from the kernel's entry they would be spilled across the scan, which needs them all
    __shared__ Tex sharedTex;
    __shared__ AlphaInputs sharedAlpha; // the alpha-tested scan's, for the same reason
    __shared__ Candidate candidates[4][kCandidateSlots];           // } per wave (the alpha-tested kernel only): AlphaScan
    __shared__ uint32_t alphaRecords[4][kAlphaRecordWords][64];    // }
    if constexpr (kTextured) {
        if (threadIdx.x == 0) {
            static_cast<TextureInputs&>(sharedTex) = p.tex;
            if constexpr (kFormats) sharedTex.formats = p.formats;
            if constexpr (kAniso) sharedTex.maxAnisotropy = p.maxAnisotropy;
        }
    }
    // the alpha-tested kernel takes ALL its arguments from LDS: its scan needs the resolve's buffers too, and held in scalar registers from the kernel's entry
    // thirty of them were spilled
    __shared__ Params sharedParams;
    if constexpr (kAlphaTest) {
        if (threadIdx.x == 0) { sharedAlpha = AlphaInputs{p.alphaCutoffs, p.global->mipBias}; sharedParams = p; }
    }
    __syncthreads();
    const Params& q = *(kAlphaTest ? &sharedParams : &p);
    const uint32_t n = min(q.header->cursor, q.capacity);
    const rastercov::TileWindow window{tx, ty, ox, oy, min(ox + kTileSize - 1, q.width - 1), min(oy + kTileSize - 1, q.height - 1)};
    if constexpr (kAlphaTest) {
        AlphaWalk<Tex> walk{AlphaScan<Tex>{candidates[wave], alphaRecords[wave], &sharedTex, 0.f, 0, 0, tile, ox, oy, lane, 0u}, &q, &sharedAlpha, kAlphaCutoffOpaque, kAlphaCutoffOpaque};
        rastercov::rasteriseTile(q.rects, q.records, n, window, hitQueue[wave], walk);
    } else {
        KeyWalk walk{{}, tile, ox, oy};
        rastercov::rasteriseTile(q.rects, q.records, n, window, hitQueue[wave], walk);
    }
    __syncthreads();
    // resolve: a lane per pixel, a wave per tile row - 64 four-byte texels, 256 contiguous bytes of every image per store instruction
    Tex tex{};
    if constexpr (kTextured) tex = sharedTex;
    for (uint32_t i = threadIdx.x; i < (uint32_t)(kTileSize * kTileSize); i += 256u) {
        const int y = oy + (int)(i >> 6), x = ox + (int)(i & 63u);
        if (y >= q.height || x >= q.width) continue;
        const Key key = tile[i];
        uint32_t motion = 0u, normal = 0u, albedo = 0u, specular = 0u;
        const uint32_t t = (uint32_t)key;
        const bool winner = key != 0ull && t < q.triangleCount;
        if (winner) resolvePixel<kTextured, Tex>(q, tex, t, x, y, &motion, &normal, &albedo, &specular);
        const size_t at = (size_t)y * (size_t)q.width + (size_t)x;
        q.depth[at] = u2f((uint32_t)(key >> 32));
        q.motion[at] = motion; q.normal[at] = normal; q.albedo[at] = albedo; q.specular[at] = specular;
        if constexpr (kNormalMap) q.shadingNormal[at] = winner ? t : kNoWinner;
    }
}

// ---- normal maps (the normal map contract)
struct ShadingNormalParams {
    const TriangleOrigin* origins; const float* transforms; const float* positions; const float* normals; const uint32_t* indices; const Draw* draws;
    const GlobalUbo* global;
    const uint32_t* normal;  // what the tile kernel stored: a pixel without a normal map, and one whose M does not normalise, takes this word
    uint32_t* shadingNormal; // in: the winner's t or kNoWinner; out: the shading normal
    const float* tangents; const float* bitangents; const uint32_t* normalMaterials;
    uint64_t tangentVertexCount, bitangentVertexCount;
    uint32_t triangleCount, normalMaterialCount, decode;
    int32_t width, height;
    int32_t windowX0, windowY0; // the window's first pixel: the grid covers the window's rows and columns (0, 0 without a window)
    TextureInputs tex;
};

PLR_DI D3 fetchBasisVector(const float* buffer, uint64_t vertexCount, uint64_t vertex) { // a vertex outside the buffer has (0, 0, 0)
    if (vertex >= vertexCount) return D3{0.0, 0.0, 0.0};
    return D3{(double)buffer[vertex * 3u], (double)buffer[vertex * 3u + 1u], (double)buffer[vertex * 3u + 2u]};
}

// n_s of triangle origins[t] = o at pixel (x, y) with the usable normal texture `texture`, as the stored word; `fallback` where M does not normalise
template <bool kFormats, bool kAniso = false>
PLR_DI uint32_t shadingNormalAt(const ShadingNormalParams& p, TriangleOrigin o, Texture texture, int x, int y, uint32_t fallback, uint32_t maxAniso = 0u) {
    const Draw draw = p.draws[o.draw];
    const uint64_t at = (uint64_t)draw.firstIndex + (uint64_t)o.local * 3u;
    const float* model = p.transforms + (size_t)draw.transformIndex * 48u;
    const float* mvp = model + 16;
    float pos[3][3], nrm[3][3];
    uint64_t vertex[3];
    fetchWinnerVertices(p.indices, p.positions, p.normals, at, draw.vertexOffset, vertex, pos, nrm);
    D3 V[3];
    for (int k = 0; k < 3; k++) V[k] = clipXYW(mvp, pos[k]);
    const D3 P{(double)(2 * x + 1) / (double)p.width - 1.0, (double)(2 * y + 1) / (double)p.height - 1.0, 1.0};
    double b[3];
    barycentricsAt(P, V, b);
    // the texel: the sampling contract's word, through the albedo sampler's own functions
    double tu[3], tv[3];
    for (int k = 0; k < 3; k++) fetchUv(p.tex, vertex[k], &tu[k], &tv[k]);
    const UvSample uv = uvSampleAt<kAniso>(P, b, V, tu, tv, x, y, p.width, p.height);
    const uint32_t texel = sampleTexture<0, kFormats, kAniso>(p.tex, texture, uv.u, uv.v, uv.dudx, uv.dvdx, uv.dudy, uv.dvdy, p.global->mipBias, maxAniso);
    const double cx = (double)(texel & 255u) / 255.0, cy = (double)((texel >> 8) & 255u) / 255.0;
    D3 nt;
    if (p.decode == kNormalDecodeReference) {
        const double z = __builtin_sqrt(((1.0 - cx * cx) + cy) + cy); // (the reference's expression as written)
        nt = D3{2.0 * cx - 1.0, 2.0 * cy - 1.0, 2.0 * z - 1.0};
    } else {
        const double nx = 2.0 * cx - 1.0, ny = 2.0 * cy - 1.0;
        const double q = (1.0 - nx * nx) - ny * ny;
        nt = D3{nx, ny, q > 0.0 ? __builtin_sqrt(q) : 0.0};
    }
    // the interpolated basis, not renormalised
    D3 N[3];
    vertexNormals(pos, nrm, model, N);
    D3 M{0.0, 0.0, 0.0};
    {
        D3 T[3], B[3];
        for (int k = 0; k < 3; k++) {
            T[k] = normalized(rotated(model, fetchBasisVector(p.tangents, p.tangentVertexCount, vertex[k])));
            B[k] = normalized(rotated(model, fetchBasisVector(p.bitangents, p.bitangentVertexCount, vertex[k])));
        }
        const D3 Ti{weighted(b, T[0].x, T[1].x, T[2].x), weighted(b, T[0].y, T[1].y, T[2].y), weighted(b, T[0].z, T[1].z, T[2].z)};
        const D3 Bi{weighted(b, B[0].x, B[1].x, B[2].x), weighted(b, B[0].y, B[1].y, B[2].y), weighted(b, B[0].z, B[1].z, B[2].z)};
        const D3 Nv{weighted(b, N[0].x, N[1].x, N[2].x), weighted(b, N[0].y, N[1].y, N[2].y), weighted(b, N[0].z, N[1].z, N[2].z)};
        M = D3{(Ti.x * nt.x + Bi.x * nt.y) + Nv.x * nt.z, (Ti.y * nt.x + Bi.y * nt.y) + Nv.y * nt.z, (Ti.z * nt.x + Bi.z * nt.y) + Nv.z * nt.z};
    }
    const D3 ns = normalized(M);
    if (ns.x == 0.0 && ns.y == 0.0 && ns.z == 0.0) return fallback; // the Normal rule's n: the word behind `normal`
    return unorm8Half((float)ns.x) | (unorm8Half((float)ns.y) << 8) | (unorm8Half((float)ns.z) << 16) | (255u << 24);
}

// A lane per pixel, a wave per 64 consecutive pixels of one row (256 contiguous bytes read and stored), in place: a lane reads the t the tile kernel left in its
// texel and overwrites that texel. No LDS, no atomics. A wave of sky only, and a wave none of whose draws has a usable normal texture, leave by a ballot.
struct FormatShadingNormalParams : ShadingNormalParams { const uint32_t* formats; };
struct AnisoShadingNormalParams : FormatShadingNormalParams { uint32_t maxAnisotropy; };
template <bool kFormats, bool kAniso = false> struct ShadingNormalParamsOf { typedef ShadingNormalParams type; };
template <> struct ShadingNormalParamsOf<true, false> { typedef FormatShadingNormalParams type; };
template <> struct ShadingNormalParamsOf<true, true> { typedef AnisoShadingNormalParams type; };

template <bool kFormats = false, bool kAniso = false>
__global__ __launch_bounds__(256) void depthPrepassShadingNormalKernel(typename ShadingNormalParamsOf<kFormats, kAniso>::type p) {
    static_assert(kFormats || !kAniso, "the anisotropic instantiation exists in the format-aware form only");
    const int x = p.windowX0 + (int)(blockIdx.x * 64u + (threadIdx.x & 63u)), y = p.windowY0 + (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (y >= p.height) return; // (wave-uniform)
    const bool inside = x < p.width;
    const size_t at = (size_t)y * (size_t)p.width + (size_t)(inside ? x : 0);
    const uint32_t t = inside ? p.shadingNormal[at] : kNoWinner;
    const bool winner = t < p.triangleCount;
    uint32_t word = 0u;
    if (__ballot(winner) != 0ull) {
        TriangleOrigin o{0u, 0u};
        Texture texture{};
        bool mapped = false;
        if (winner) {
            word = p.normal[at];
            o = p.origins[t];
            if (o.draw < p.tex.drawCount && o.draw < p.normalMaterialCount) {
                if constexpr (kAniso) {
                    AnisoTextureInputs tex;
                    static_cast<TextureInputs&>(tex) = p.tex;
                    tex.formats = p.formats;
                    mapped = usableTexture(tex, p.normalMaterials[o.draw], &texture);
                } else if constexpr (kFormats) {
                    FormatTextureInputs tex;
                    static_cast<TextureInputs&>(tex) = p.tex;
                    tex.formats = p.formats;
                    mapped = usableTexture(tex, p.normalMaterials[o.draw], &texture);
                } else
                    mapped = usableTexture(p.tex, p.normalMaterials[o.draw], &texture);
            }
        }
        if constexpr (kAniso) {
            if (__ballot(mapped) != 0ull && mapped) word = shadingNormalAt<true, true>(p, o, texture, x, y, word, p.maxAnisotropy);
        } else if (__ballot(mapped) != 0ull && mapped) word = shadingNormalAt<kFormats>(p, o, texture, x, y, word);
    }
    if (inside) p.shadingNormal[at] = word;
}

static int launchDepthPrepassRaster(const PassCtx& c) {
    if (c.push.size() < sizeof(PushConstants)) return c.fail(-1, "depthPrepassRaster: push constants {drawCount, triangleCount} missing");
    if (!pushSizeDefined(c.push.size()))
        return c.fail(-1, "depthPrepassRaster: the push constants are " + std::to_string(c.push.size()) + " bytes, the record has 8, 12, 16, 20, 24, 28 or 44 (words 0 - 6, or all of them and the tile window)");
    WindowPushConstants pc{};
    std::memcpy(&pc, c.push.data(), c.push.size()); // 8 bytes: {drawCount, triangleCount}, textureCount 0; 12: alphaTest 0; 16: normalMap 0; 20: textureFormats 0; 24: maxAnisotropy 0; 28: no window
    const bool windowed = c.push.size() == sizeof(WindowPushConstants);
    const bool aniso = pc.maxAnisotropy >= 2u; // 0 and 1: the isotropic pass, word for word
    if (c.dispatch[0] != 1u || c.dispatch[1] != 1u || c.dispatch[2] != 1u || c.base[0] != 0u || c.base[1] != 0u)
        return c.fail(-1, "depthPrepassRaster: the dispatch is {1, 1, 1} (the launcher derives its grids from the push constants and the images)");
    if (pc.triangleCount > kMaxTriangles) return c.fail(-1, "depthPrepassRaster: triangleCount " + std::to_string(pc.triangleCount) + " exceeds 2^28");
    if ((pc.drawCount == 0u) != (pc.triangleCount == 0u)) return c.fail(-1, "depthPrepassRaster: drawCount and triangleCount must both be zero or both be non-zero");
    if (int rc = c.needGlobal()) return rc;
    if (int rc = c.needSbuf(kTransformBinding, 0, "depthPrepassRaster transforms (MainPassMatrices[]: model, mvp, mvpPrevious)")) return rc;
    if (int rc = c.needSbuf(kPositionBinding, 0, "depthPrepassRaster positions (3 floats per vertex)")) return rc;
    if (int rc = c.needSbuf(kNormalBinding, 0, "depthPrepassRaster normals (3 floats per vertex)")) return rc;
    if (int rc = c.needSbuf(kIndexBinding, 0, "depthPrepassRaster indices (uint32 triangle list)")) return rc;
    if (int rc = c.needSbuf(kDrawBinding, (size_t)pc.drawCount * sizeof(Draw), "depthPrepassRaster draws {firstIndex, indexCount, vertexOffset, transformIndex, albedo, specular}")) return rc;
    if (int rc = c.needSbuf(kScratchBinding, scratchBytes(pc.triangleCount),
                            "depthPrepassRaster scratch (align16(align16(64 + 8 triangleCount) + 24 triangleCount) + 576 triangleCount bytes: 6 sub-triangles per triangle)"))
        return rc;
    if (pc.textureCount) {
        if (int rc = c.needSbuf(kUvBinding, 0, "depthPrepassRaster uvs (2 floats per vertex)")) return rc;
        if (int rc = c.needSbuf(kMaterialBinding, (size_t)pc.drawCount * sizeof(Material), "depthPrepassRaster materials {albedoTexture, specularTexture} per draw")) return rc;
        if (int rc = c.needSbuf(kTextureBinding, (size_t)pc.textureCount * sizeof(Texture), "depthPrepassRaster textures {texelOffset, width, height, mipCount}")) return rc;
        if (int rc = c.needSbuf(kTexelBinding, 0, "depthPrepassRaster texels (RGBA8, every texture's levels back to back)")) return rc;
    }
    if (pc.alphaTest) {
        if (pc.textureCount == 0u) return c.fail(-1, "depthPrepassRaster: alphaTest is set and textureCount is 0 (the alpha of a fragment is its albedo sample: the alpha test needs textures)");
        if (int rc = c.needSbuf(kAlphaCutoffBinding, (size_t)pc.drawCount * 4u, "depthPrepassRaster alphaCutoffs (one uint32 cutoff code per draw)")) return rc;
    }
    if (pc.normalMap) {
        if (pc.normalMap != kNormalDecodeReference && pc.normalMap != kNormalDecodeUnit)
            return c.fail(-1, "depthPrepassRaster: normalMap is " + std::to_string(pc.normalMap) + ", it must be 0 (none), 1 (the reference's decode) or 2 (the unit decode)");
        if (pc.textureCount == 0u) return c.fail(-1, "depthPrepassRaster: normalMap is set and textureCount is 0 (a normal map is a texture of the texture store: normal maps need textures)");
        if (int rc = c.needSbuf(kTangentBinding, 0, "depthPrepassRaster tangents (3 floats per vertex)")) return rc;
        if (int rc = c.needSbuf(kBitangentBinding, 0, "depthPrepassRaster bitangents (3 floats per vertex)")) return rc;
        if (int rc = c.needSbuf(kNormalMaterialBinding, (size_t)pc.drawCount * 4u, "depthPrepassRaster normalMaterials (one uint32 texture index per draw)")) return rc;
    }
    if (pc.textureFormats) {
        if (pc.textureFormats != 1u)
            return c.fail(-1, "depthPrepassRaster: textureFormats is " + std::to_string(pc.textureFormats) + ", it must be 0 (every texture is RGBA8) or 1 (binding 14 holds a format code per texture)");
        if (pc.textureCount == 0u) return c.fail(-1, "depthPrepassRaster: textureFormats is set and textureCount is 0 (a format belongs to a texture of the texture store)");
        if (int rc = c.needSbuf(kTextureFormatBinding, (size_t)pc.textureCount * 4u, "depthPrepassRaster textureFormats (binding 14: one uint32 format code per texture)")) return rc;
        if (c.sbuf[kTextureFormatBinding].ptr == c.sbuf[kScratchBinding].ptr)
            return c.fail(-4, "depthPrepassRaster: the scratch buffer is also bound as an input (binding 14, textureFormats)");
    }
    if (aniso) {
        if (pc.maxAnisotropy > kMaxAnisotropy)
            return c.fail(-1, "depthPrepassRaster: maxAnisotropy is " + std::to_string(pc.maxAnisotropy) + ", it must be 0 or 1 (isotropic trilinear filtering) or 2 .. 16 (the probe count's upper bound)");
        if (pc.textureCount == 0u) return c.fail(-1, "depthPrepassRaster: maxAnisotropy is set and textureCount is 0 (anisotropic filtering is a property of the texture samples: it needs textures)");
    }
    if (c.sbuf[kScratchBinding].readOnly) return c.fail(-4, "depthPrepassRaster: the scratch buffer (binding 5) is bound read-only");
    if (int rc = c.needStorage(kDepthBinding, F_D32, "depthPrepassRaster depth")) return rc;
    if (int rc = c.needStorage(kMotionBinding, F_RG16SN, "depthPrepassRaster motion")) return rc;
    if (int rc = c.needStorage(kNormalImageBinding, F_RGBA8, "depthPrepassRaster world-space normal")) return rc;
    if (int rc = c.needStorage(kAlbedoBinding, F_RGBA8, "depthPrepassRaster albedo")) return rc;
    if (int rc = c.needStorage(kSpecularBinding, F_RGBA8, "depthPrepassRaster specular")) return rc;
    const ImgView depth = c.storage[kDepthBinding];
    if (depth.w < 1 || depth.h < 1 || depth.w > kMaxResolution || depth.h > kMaxResolution || depth.d > 1)
        return c.fail(-4, "depthPrepassRaster: the depth image is " + std::to_string(depth.w) + " x " + std::to_string(depth.h) + ", it must be 2D and at most 16384 x 16384");
    for (int b : {kMotionBinding, kNormalImageBinding, kAlbedoBinding, kSpecularBinding}) {
        if (c.storage[b].w != depth.w || c.storage[b].h != depth.h || c.storage[b].d > 1)
            return c.fail(-4, "depthPrepassRaster: the five images must have one size; storage binding " + std::to_string(b) + " is " + std::to_string(c.storage[b].w) + " x " +
                                  std::to_string(c.storage[b].h) + ", depth is " + std::to_string(depth.w) + " x " + std::to_string(depth.h));
        for (int o = 0; o < b; o++)
            if (c.storage[o].ptr == c.storage[b].ptr) return c.fail(-4, "depthPrepassRaster: one image is bound at two storage bindings");
    }
    for (int b : {kTransformBinding, kPositionBinding, kNormalBinding, kIndexBinding, kDrawBinding})
        if (c.sbuf[b].ptr == c.sbuf[kScratchBinding].ptr) return c.fail(-4, "depthPrepassRaster: the scratch buffer is also bound as an input");
    if (pc.textureCount)
        for (int b : {kUvBinding, kMaterialBinding, kTextureBinding, kTexelBinding})
            if (c.sbuf[b].ptr == c.sbuf[kScratchBinding].ptr) return c.fail(-4, "depthPrepassRaster: the scratch buffer is also bound as an input");
    if (pc.alphaTest && c.sbuf[kAlphaCutoffBinding].ptr == c.sbuf[kScratchBinding].ptr)
        return c.fail(-4, "depthPrepassRaster: the scratch buffer is also bound as an input (binding 10, alphaCutoffs)");
    if (pc.normalMap) {
        if (int rc = c.needStorage(kShadingNormalBinding, F_RGBA8, "depthPrepassRaster shadingNormal")) return rc;
        const ImgView sn = c.storage[kShadingNormalBinding];
        if (sn.w != depth.w || sn.h != depth.h || sn.d > 1)
            return c.fail(-4, "depthPrepassRaster: shadingNormal (storage binding 5) is " + std::to_string(sn.w) + " x " + std::to_string(sn.h) + ", it must have the size of the other five: depth is " +
                                  std::to_string(depth.w) + " x " + std::to_string(depth.h));
        for (int o = 0; o < kShadingNormalBinding; o++)
            if (c.storage[o].ptr == sn.ptr) return c.fail(-4, "depthPrepassRaster: one image is bound at two storage bindings (shadingNormal, binding 5)");
        for (int b : {kTangentBinding, kBitangentBinding, kNormalMaterialBinding})
            if (c.sbuf[b].ptr == c.sbuf[kScratchBinding].ptr)
                return c.fail(-4, "depthPrepassRaster: the scratch buffer is also bound as an input (binding " + std::to_string(b) + ", a normal map input)");
    }
    // the tile window: the whole grid without one (every shorter record), and then today's grids
    const uint32_t gridX = divUp((unsigned)depth.w, (unsigned)kTileSize), gridY = divUp((unsigned)depth.h, (unsigned)kTileSize);
    uint32_t wx0 = 0u, wy0 = 0u, wx1 = gridX, wy1 = gridY;
    if (windowed) {
        const std::string given = "{" + std::to_string(pc.windowTileX0) + ", " + std::to_string(pc.windowTileY0) + ", " + std::to_string(pc.windowTileX1) + ", " + std::to_string(pc.windowTileY1) + "}";
        if (pc.windowTileX0 >= pc.windowTileX1 || pc.windowTileY0 >= pc.windowTileY1)
            return c.fail(-1, "depthPrepassRaster: the tile window " + given + " is empty or inverted (it is half-open: x0 < x1 and y0 < y1)");
        if (pc.windowTileX1 > gridX || pc.windowTileY1 > gridY)
            return c.fail(-1, "depthPrepassRaster: the tile window " + given + " reaches past the tile grid of the bound images, " + std::to_string(gridX) + " x " + std::to_string(gridY) +
                                  " tiles of 64 x 64 (" + std::to_string(depth.w) + " x " + std::to_string(depth.h) + " pixels)");
        wx0 = pc.windowTileX0; wy0 = pc.windowTileY0; wx1 = pc.windowTileX1; wy1 = pc.windowTileY1;
    }

    uint8_t* scratch = (uint8_t*)c.sbuf[kScratchBinding].ptr;
    if (hipMemsetAsync(scratch, 0, sizeof(ScratchHeader), c.stream) != hipSuccess) return c.fail(-2, "depthPrepassRaster: clearing the scratch header failed");
    const uint32_t capacity = pc.triangleCount * kMaxSubTriangles;
    if (pc.triangleCount) {
        SetupParams s{};
        s.transforms = (const float*)c.sbuf[kTransformBinding].ptr; s.positions = (const float*)c.sbuf[kPositionBinding].ptr;
        s.indices = (const uint32_t*)c.sbuf[kIndexBinding].ptr; s.draws = (const Draw*)c.sbuf[kDrawBinding].ptr;
        s.header = (ScratchHeader*)scratch; s.origins = (TriangleOrigin*)(scratch + originOffset());
        s.rects = (uint32_t*)(scratch + rectOffset(pc.triangleCount)); s.records = (Record*)(scratch + recordOffset(pc.triangleCount));
        s.drawCount = pc.drawCount; s.triangleCount = pc.triangleCount; s.capacity = capacity;
        s.transformCount = (uint32_t)std::min<size_t>(c.sbuf[kTransformBinding].size / sizeof(MainPassMatrices), 0xffffffffu);
        s.vertexCount = (uint32_t)std::min<size_t>(std::min(c.sbuf[kPositionBinding].size, c.sbuf[kNormalBinding].size) / 12u, 0xffffffffu);
        s.indexCount = (uint32_t)std::min<size_t>(c.sbuf[kIndexBinding].size / 4u, 0xffffffffu);
        s.width = depth.w; s.height = depth.h;
        s.window = wx0 | (wy0 << 8) | ((wx1 - 1u) << 16) | ((wy1 - 1u) << 24); // (the grid is at most 256 x 256 tiles)
        depthPrepassSetupKernel<<<divUp(pc.triangleCount, 256u), 256, 0, c.stream>>>(s);
        PLR_CHECK_LAUNCH(c);
        c.splitTiming("set-up");
    }
    TileParams t{};
    t.header = (ScratchHeader*)scratch; t.origins = (const TriangleOrigin*)(scratch + originOffset());
    t.rects = (const uint32_t*)(scratch + rectOffset(pc.triangleCount)); t.records = (const Record*)(scratch + recordOffset(pc.triangleCount));
    t.transforms = (const float*)c.sbuf[kTransformBinding].ptr; t.positions = (const float*)c.sbuf[kPositionBinding].ptr; t.normals = (const float*)c.sbuf[kNormalBinding].ptr;
    t.indices = (const uint32_t*)c.sbuf[kIndexBinding].ptr; t.draws = (const Draw*)c.sbuf[kDrawBinding].ptr;
    t.global = c.global;
    t.depth = (float*)depth.ptr; t.motion = (uint32_t*)c.storage[kMotionBinding].ptr; t.normal = (uint32_t*)c.storage[kNormalImageBinding].ptr;
    t.albedo = (uint32_t*)c.storage[kAlbedoBinding].ptr; t.specular = (uint32_t*)c.storage[kSpecularBinding].ptr;
    t.capacity = capacity; t.triangleCount = pc.triangleCount; t.width = depth.w; t.height = depth.h;
    t.windowTileX0 = (int32_t)wx0; t.windowTileY0 = (int32_t)wy0;
    const dim3 tiles(wx1 - wx0, wy1 - wy0);
    if (pc.textureCount) {
        t.tex.uvs = (const float*)c.sbuf[kUvBinding].ptr; t.tex.materials = (const Material*)c.sbuf[kMaterialBinding].ptr;
        t.tex.textures = (const Texture*)c.sbuf[kTextureBinding].ptr; t.tex.texels = (const uint32_t*)c.sbuf[kTexelBinding].ptr;
        t.tex.uvVertexCount = c.sbuf[kUvBinding].size / 8u; t.tex.texelCount = c.sbuf[kTexelBinding].size / 4u;
        t.tex.drawCount = pc.drawCount; t.tex.textureCount = pc.textureCount;
        const uint32_t* formats = pc.textureFormats ? (const uint32_t*)c.sbuf[kTextureFormatBinding].ptr : nullptr; // only then the format-aware instantiations run
        if (pc.alphaTest) t.alphaCutoffs = (const uint32_t*)c.sbuf[kAlphaCutoffBinding].ptr;
        if (pc.normalMap) {
            NormalTileParams n{};
            static_cast<TileParams&>(n) = t;
            n.shadingNormal = (uint32_t*)c.storage[kShadingNormalBinding].ptr;
            if (aniso) { // format-aware whatever textureFormats says: a null `formats` makes every texture RGBA8
                AnisoNormalTileParams a{};
                static_cast<NormalTileParams&>(a) = n;
                a.formats = formats; a.maxAnisotropy = pc.maxAnisotropy;
                if (pc.alphaTest) depthPrepassTileKernel<true, true, true, true, true><<<tiles, 256, 0, c.stream>>>(a);
                else depthPrepassTileKernel<true, false, true, true, true><<<tiles, 256, 0, c.stream>>>(a);
            } else if (formats) {
                FormatNormalTileParams f{};
                static_cast<NormalTileParams&>(f) = n;
                f.formats = formats;
                if (pc.alphaTest) depthPrepassTileKernel<true, true, true, true><<<tiles, 256, 0, c.stream>>>(f);
                else depthPrepassTileKernel<true, false, true, true><<<tiles, 256, 0, c.stream>>>(f);
            } else if (pc.alphaTest)
                depthPrepassTileKernel<true, true, true><<<tiles, 256, 0, c.stream>>>(n);
            else
                depthPrepassTileKernel<true, false, true><<<tiles, 256, 0, c.stream>>>(n);
            PLR_CHECK_LAUNCH(c);
            c.splitTiming("tiles");
            AnisoShadingNormalParams s{};
            s.origins = t.origins; s.transforms = t.transforms; s.positions = t.positions; s.normals = t.normals; s.indices = t.indices; s.draws = t.draws;
            s.global = c.global; s.normal = t.normal; s.shadingNormal = n.shadingNormal;
            s.tangents = (const float*)c.sbuf[kTangentBinding].ptr; s.bitangents = (const float*)c.sbuf[kBitangentBinding].ptr;
            s.normalMaterials = (const uint32_t*)c.sbuf[kNormalMaterialBinding].ptr;
            s.tangentVertexCount = c.sbuf[kTangentBinding].size / 12u; s.bitangentVertexCount = c.sbuf[kBitangentBinding].size / 12u;
            s.triangleCount = pc.triangleCount; s.normalMaterialCount = (uint32_t)std::min<size_t>(c.sbuf[kNormalMaterialBinding].size / 4u, 0xffffffffu);
            s.decode = pc.normalMap; s.width = depth.w; s.height = depth.h; s.tex = t.tex;
            s.formats = formats; s.maxAnisotropy = pc.maxAnisotropy;
            s.windowX0 = (int32_t)(wx0 * (uint32_t)kTileSize); s.windowY0 = (int32_t)(wy0 * (uint32_t)kTileSize);
            // the window's columns and rows (the kernel drops what lies past the image's last row and column)
            const dim3 rows(wx1 - wx0, divUp(std::min((unsigned)depth.h, wy1 * (unsigned)kTileSize) - wy0 * (unsigned)kTileSize, 4u));
            if (aniso) depthPrepassShadingNormalKernel<true, true><<<rows, 256, 0, c.stream>>>(s);
            else if (formats) depthPrepassShadingNormalKernel<true><<<rows, 256, 0, c.stream>>>(static_cast<const FormatShadingNormalParams&>(s));
            else depthPrepassShadingNormalKernel<false><<<rows, 256, 0, c.stream>>>(static_cast<const ShadingNormalParams&>(s));
        } else if (aniso) {
            AnisoTileParams a{};
            static_cast<TileParams&>(a) = t;
            a.formats = formats; a.maxAnisotropy = pc.maxAnisotropy;
            if (pc.alphaTest) depthPrepassTileKernel<true, true, false, true, true><<<tiles, 256, 0, c.stream>>>(a);
            else depthPrepassTileKernel<true, false, false, true, true><<<tiles, 256, 0, c.stream>>>(a);
        } else if (formats) {
            FormatTileParams f{};
            static_cast<TileParams&>(f) = t;
            f.formats = formats;
            if (pc.alphaTest) depthPrepassTileKernel<true, true, false, true><<<tiles, 256, 0, c.stream>>>(f);
            else depthPrepassTileKernel<true, false, false, true><<<tiles, 256, 0, c.stream>>>(f);
        } else if (pc.alphaTest)
            depthPrepassTileKernel<true, true><<<tiles, 256, 0, c.stream>>>(t);
        else
            depthPrepassTileKernel<true><<<tiles, 256, 0, c.stream>>>(t);
    } else
        depthPrepassTileKernel<false><<<tiles, 256, 0, c.stream>>>(t);
    PLR_CHECK_LAUNCH(c);
    return 0;
}

} // namespace prepass
static int depth_prepass_raster_launch(const PassCtx& c) { return prepass::launchDepthPrepassRaster(c); }
static int depth_prepass_raster_launch_fast(const PassCtx& c) { return prepass::launchDepthPrepassRaster(c); }
PLR_REGISTER_SHADER("depthPrepassRaster.comp", depth_prepass_raster_launch);
PLR_REGISTER_SHADER_FAST("depthPrepassRaster.comp", depth_prepass_raster_launch_fast);
} // namespace plr
