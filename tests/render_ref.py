"""Helper of the renderer's tests (not a test module): a numpy oracle written from the renderer's specification, not
from the kernel, and the synthetic closed meshes the tests draw.

The oracle works on GIVEN fixed-point coordinates (1/256 px): int64 coverage at pixel centres with the top-left rule, fp64 depth, normals
and shading, and per pixel the list of surviving fragments.  A pixel is DECIDED when its nearest and second-nearest surviving fragments
differ in z by more than TAU and no candidate fragment lies within TAU of a clip plane.  TAU = 1e-5: the kernel interpolates z in fp32
with three products, two sums and a division on |z| <= 1, each within 2^-24 relative - an error below 1e-6, so TAU carries a 10 x margin."""
import numpy as np

TAU = 1e-5
SUB = 256
GUARD = (1 << 14) * SUB
COLOR = (1.0, 0.6059142480254321, 0.5)
EMISSIVE, AMBIENT, INTENSITY = 0.1, 0.3, 1.2
LIGHTS = np.array([[0.0, -np.sqrt(0.5), -np.sqrt(0.5)], [np.sqrt(0.5), 0.0, -np.sqrt(0.5)]])
RX = np.diag([1.0, -1.0, -1.0])


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def _outward(verts, faces):
    """Wind every face so that (b - a) x (c - a) points away from the origin (the meshes are star-shaped around it)."""
    a, b, c = (verts[faces[:, i]] for i in range(3))
    flip = np.einsum("ij,ij->i", np.cross(b - a, c - a), a + b + c) < 0
    faces = faces.copy()
    faces[flip] = faces[flip][:, [0, 2, 1]]
    return faces


def icosphere(subdiv: int = 2):
    """Unit icosphere: 162 vertices and 320 faces at two subdivisions; outward winding."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = np.array(v)
    return verts, _outward(verts, np.array(f, dtype=np.int32))


def uv_sphere(rings: int = 83, segments: int = 84):
    """Unit UV sphere; 83 x 84 gives exactly 6890 vertices and 13 776 faces (SMPL's counts); outward winding."""
    th = np.pi * np.arange(1, rings) / rings
    ph = 2 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.cos(th), np.ones(segments)), np.outer(np.sin(th), np.sin(ph))], -1)
    verts = np.concatenate([[[0.0, 1.0, 0.0]], ring.reshape(-1, 3), [[0.0, -1.0, 0.0]]])
    idx = lambda r, s: 1 + r * segments + (s % segments)  # noqa: E731
    f = []
    for s in range(segments):
        f.append((0, idx(0, s), idx(0, s + 1)))
        f.append((len(verts) - 1, idx(rings - 2, s + 1), idx(rings - 2, s)))
        for r in range(rings - 2):
            f.append((idx(r, s), idx(r + 1, s), idx(r + 1, s + 1)))
            f.append((idx(r, s), idx(r + 1, s + 1), idx(r, s + 1)))
    return verts, _outward(verts, np.array(f, dtype=np.int32))


BODY = (0.25, 0.85, 0.15)      # semi-axes in metres: an ellipsoid of body proportions


def ellipsoid(mesh, axes=BODY, centre=(0.0, 0.0, 0.0)):
    verts, faces = mesh
    return (verts * np.asarray(axes) + np.asarray(centre)).astype(np.float32), faces


def two_ellipsoids(mesh):
    """ONE mesh of two interpenetrating ellipsoids: their surfaces cross along a curve, the only place two fragments meet in depth."""
    v1, f = ellipsoid(mesh, BODY, (-0.08, 0.0, 0.0))
    v2, _ = ellipsoid(mesh, (0.2, 0.6, 0.2), (0.12, 0.1, 0.05))
    return np.concatenate([v1, v2]), np.concatenate([f, f + len(v1)]).astype(np.int32)


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def transform(verts, rotation=None):
    """fp64 vertices in the model's frame after the reference's rotation of the flipped mesh: q = Rx R Rx p."""
    p = np.asarray(verts, dtype=np.float64)
    return p if rotation is None else p @ (RX @ np.asarray(rotation, dtype=np.float64) @ RX).T


def project(q, cam, W, H):
    """fp64 pixel coordinates [V,2], origin at the top-left corner, y down."""
    sx, sy, tx, ty = (float(c) for c in cam)
    return np.stack([(sx * (q[:, 0] + tx) + 1.0) * W / 2.0, (sy * (q[:, 1] + ty) + 1.0) * H / 2.0], -1)


def snap(uv):
    return np.rint(np.asarray(uv, dtype=np.float64) * SUB).astype(np.int64)


def fragments(xy, z, faces, W, H, cull=True):
    """All candidate fragments of a mesh on fixed-point coordinates xy int[V,2] with depths z[V] (fp64): a dict of flat arrays
    (y, x, face, z, w[.,3] barycentric weights of the face's three vertices) BEFORE clipping, plus 'guard': a triangle was dropped."""
    xy = np.asarray(xy, dtype=np.int64)
    out = {k: [] for k in ("y", "x", "face", "z", "w")}
    guard = False
    for f, (ia, ib, ic) in enumerate(np.asarray(faces)):
        P = xy[[ia, ib, ic]]
        if np.abs(P).max() > GUARD:
            guard = True
            continue
        (ax, ay), (bx, by), (cx, cy) = (tuple(int(t) for t in p) for p in P)
        area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
        if area == 0 or (cull and area > 0):        # front faces have their winding normal along -z: negative area, y down
            continue
        # pixel columns / rows whose centres lie inside the bounding box
        x0, x1 = max(0, -((-(P[:, 0].min() - 128)) // 256)), min(W - 1, (P[:, 0].max() - 128) // 256)
        y0, y1 = max(0, -((-(P[:, 1].min() - 128)) // 256)), min(H - 1, (P[:, 1].max() - 128) // 256)
        if x1 < x0 or y1 < y0:
            continue
        sx = (np.arange(x0, x1 + 1, dtype=np.int64) * 256 + 128)[None, :]
        sy = (np.arange(y0, y1 + 1, dtype=np.int64) * 256 + 128)[:, None]
        sgn = 1 if area > 0 else -1
        inside = np.ones((sy.size, sx.size), dtype=bool)
        ws = []
        for (px, py), (qx, qy) in (((bx, by), (cx, cy)), ((cx, cy), (ax, ay)), ((ax, ay), (bx, by))):
            # E(s) = gx * s.x + gy * s.y + c, positive inside
            gx, gy = -sgn * (qy - py), sgn * (qx - px)
            E = gx * (sx - px) + gy * (sy - py)
            owns_edge = gx > 0 or (gx == 0 and gy > 0)      # a left edge (interior at larger x) or a top edge (interior below)
            inside &= (E > 0) | ((E == 0) & owns_edge)
            ws.append(E)
        yy, xx = np.nonzero(inside)
        if yy.size == 0:
            continue
        E = np.stack([e[yy, xx] for e in ws], -1).astype(np.float64)       # exact: |E| < 2^48
        w = E / abs(area)
        out["y"].append(yy + y0)
        out["x"].append(xx + x0)
        out["face"].append(np.full(yy.size, f, dtype=np.int64))
        out["w"].append(w)
        # the sum first, one division last: exact where the kernel's fp32 form is exact
        out["z"].append(E @ np.asarray(z, dtype=np.float64)[[ia, ib, ic]] / abs(area))
    res = {k: (np.concatenate(v) if v else np.zeros((0, 3) if k == "w" else 0, dtype=np.float64 if k in ("z", "w") else np.int64))
           for k, v in out.items()}
    res["guard"] = guard
    return res


def resolve(fr, W, H, tau=TAU):
    """Per pixel from the candidate fragments: dict of [H,W] arrays - face (-1: nothing survives), z, w [H,W,3], count (surviving
    fragments), covered (some fragment survives), clip_safe (every candidate at least tau from both clip planes), decided (covered,
    clip_safe, and the two nearest survivors more than tau apart)."""
    pix = fr["y"] * W + fr["x"]
    near_clip = np.minimum(np.abs(fr["z"] - 1.0), np.abs(fr["z"] + 1.0)) < tau
    clip_safe = np.ones(H * W, dtype=bool)
    clip_safe[pix[near_clip]] = False
    keep = (fr["z"] >= -1.0) & (fr["z"] <= 1.0)
    pix, z, face, w = pix[keep], fr["z"][keep], fr["face"][keep], fr["w"][keep]
    order = np.lexsort((face, z, pix))
    pix, z, face, w = pix[order], z[order], face[order], w[order]
    first = np.concatenate([[True], pix[1:] != pix[:-1]]) if pix.size else np.zeros(0, bool)
    count = np.bincount(pix, minlength=H * W)
    out_face = np.full(H * W, -1, dtype=np.int64)
    out_z = np.full(H * W, np.inf)
    out_w = np.zeros((H * W, 3))
    out_face[pix[first]], out_z[pix[first]], out_w[pix[first]] = face[first], z[first], w[first]
    gap_ok = np.ones(H * W, dtype=bool)
    second = np.nonzero(~first)[0]
    second = second[first[second - 1]] if second.size else second       # the fragment right after a pixel's winner
    gap_ok[pix[second]] = (z[second] - z[second - 1]) > tau
    covered = count > 0
    sh = (H, W)
    return {"face": out_face.reshape(sh), "z": out_z.reshape(sh), "w": out_w.reshape(H, W, 3), "count": count.reshape(sh),
            "covered": covered.reshape(sh), "clip_safe": clip_safe.reshape(sh), "decided": (covered & clip_safe & gap_ok).reshape(sh)}


def vertex_normals(q, faces):
    """Area-weighted: the normalised sum of the incident faces' un-normalised cross products (fp64)."""
    a, b, c = (q[faces[:, i]] for i in range(3))
    n = np.cross(b - a, c - a)
    acc = np.zeros_like(q)
    for i in range(3):
        np.add.at(acc, faces[:, i], n)
    ln = np.linalg.norm(acc, axis=1, keepdims=True)
    return np.divide(acc, ln, out=np.zeros_like(acc), where=ln > 0)


def shade(res, q, faces, color=COLOR, emissive=EMISSIVE, ambient=AMBIENT, intensity=INTENSITY, lights=LIGHTS):
    """uint8 [H,W,3] colours of the covered pixels of ``res`` (anything where nothing is covered)."""
    vn = vertex_normals(q, np.asarray(faces))
    tri = np.asarray(faces)[np.maximum(res["face"], 0)]                      # [H,W,3]
    n = np.einsum("hwk,hwkc->hwc", res["w"], vn[tri])
    ln = np.linalg.norm(n, axis=-1, keepdims=True)
    n = np.divide(n, ln, out=np.zeros_like(n), where=ln > 0)
    lsum = np.maximum(0.0, n @ np.asarray(lights, dtype=np.float64).reshape(-1, 3).T).sum(-1)
    c = emissive + (ambient + intensity / np.pi * lsum)[..., None] * np.asarray(color, dtype=np.float64)
    return np.floor(255.0 * np.clip(c, 0.0, 1.0) + 0.5).astype(np.uint8)


def draw(image, xy, verts, faces, W, H, rotation=None, cull=True, **material):
    """One job over ``image`` [H,W,3] uint8 as the specification composes it -> (image, res)."""
    q = transform(verts, rotation)
    res = resolve(fragments(xy, q[:, 2], faces, W, H, cull), W, H)
    out = image.copy()
    out[res["covered"]] = shade(res, q, faces, **material)[res["covered"]]
    return out, res


def cameras(W, H, scale=1.0):
    """Cameras (sx, sy, tx, ty) for the body-sized meshes: centred, and partly off the left, right, top and bottom edge."""
    sy = scale
    sx = sy * H / W
    return np.array([[sx, sy, 0.0, 0.0], [sx, sy, -1.0 / sx + 0.05, 0.1], [sx, sy, 1.0 / sx - 0.1, -0.05], [sx, sy, 0.03, -1.0 / sy - 0.3],
                     [sx, sy, -0.02, 1.0 / sy + 0.4]], dtype=np.float32)
