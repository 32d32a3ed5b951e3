"""Triangle meshes of refined DeepSDF shapes, extracted on the device (csrc/mesh.hip; DESIGN.md "Meshes").

    from sdflabel_amd.mesh import mesh_from_sdf, meshes_many, Mesh, load_ply, load_obj

mesh_from_sdf    the iso-surface kernels alone, on SDF samples the caller supplies on the regular lattice
meshes_many      decoder over the lattice in row chunks -> count -> ONE host read of the totals -> emit -> (polish: decoder, Jacobian and
                 Newton projection at the vertices) for a list of latents / refined parameters
Mesh             vertices / faces / normals on the device, fetched on demand; volume, area, closedness, camera frame, PLY / OBJ files

The algorithm is marching tetrahedra on the Kuhn subdivision with welded vertices: closed and consistently oriented wherever the surface
stays inside the cube.  A surface that leaves the cube [-1, 1]^3 is left OPEN at the boundary (no capping), and triangles of zero area --
they appear when the SDF is exactly 0 at lattice points -- are kept, because dropping them would open the mesh; `Mesh.faces_numpy(
drop_degenerate=True)` and `save(..., drop_degenerate=True)` filter them on the host for consumers that cannot take them.
The lattice is NOT Grid3D's staggered grid: R points per axis at float32(-1 + 2 i / (R - 1)), row = (ix R + iy) R + iz.
"""
import struct

import numpy as np
import torch

from . import _lib

R_MIN, R_MAX = 2, 256
STAGING_BYTES = 256 << 20            # default budget of the decoder's input rows in flight (a 256-wide latent at R = 128 would need 2.2 GB)


def lattice_points(R, device="cpu"):
    """[R^3][3] float32: the lattice the kernels sample, z fastest"""
    c = torch.from_numpy((-1.0 + 2.0 * np.arange(R, dtype=np.float64) / float(R - 1)).astype(np.float32))
    return torch.stack(torch.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3).to(device)


class Mesh:
    """One shape's triangle mesh.  `.vertices` float32 [V][3], `.faces` int32 [T][3] and `.normals` float32 [V][3] (or None) are device
    tensors; `*_numpy()` fetch them once, on demand.  `.scale` and `.cam_T` (4x4, as frame.assemble_labels builds it) take the lattice frame
    to the camera frame: to_camera().  `.sdf` holds the [R][R][R] samples when they were asked for.  A camera-frame mesh made by to_camera()
    carries the lattice-frame vertices it came from as `.lattice_vertices` (same order: per-vertex NOCS attributes); None otherwise."""

    def __init__(self, vertices, faces, normals=None, scale=None, cam_T=None, sdf=None, frame="lattice"):
        self.vertices, self.faces, self.normals = vertices, faces, normals
        self.scale, self.cam_T, self.sdf, self.frame = scale, cam_T, sdf, frame
        self.lattice_vertices = None
        self._host = {}

    def _fetch(self, name):
        if name not in self._host:
            t = getattr(self, name)
            self._host[name] = None if t is None else t.detach().cpu().numpy()
        return self._host[name]

    def vertices_numpy(self):
        return self._fetch("vertices")

    def normals_numpy(self):
        return self._fetch("normals")

    def faces_numpy(self, drop_degenerate=False):
        f = self._fetch("faces")
        if drop_degenerate and len(f):
            f = f[_areas(self.vertices_numpy(), f) > 0]
        return f

    def __len__(self):
        return int(self.faces.shape[0])

    def volume(self):
        """signed volume (float64 on the host): positive for an outward-wound closed mesh, in the lattice and in the camera frame alike"""
        v, f = self.vertices_numpy().astype(np.float64), self.faces_numpy()
        return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)

    def area(self):
        return float(_areas(self.vertices_numpy(), self.faces_numpy()).sum())

    def is_closed(self):
        """every undirected edge in exactly two triangles, and every directed edge matched by its reverse"""
        f = self.faces_numpy().astype(np.int64)
        if len(f) == 0:
            return False
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        n = int(f.max()) + 1
        key, cnt = np.unique(e[:, 0] * n + e[:, 1], return_counts=True)
        return bool((cnt == 1).all() and np.array_equal(key, np.unique(e[:, 1] * n + e[:, 0])))

    def to_camera(self):
        """the mesh in the camera frame: cam_T @ (scale * v).  cam_T contains diag(1, -1, 1), a reflection, so the winding is reversed and
        the normals go through the same matrix: normals still point outward and the signed volume stays positive."""
        if self.scale is None or self.cam_T is None:
            raise ValueError("Mesh.to_camera needs scale and cam_T (meshes_many sets them from refined parameters)")
        if self.frame == "camera":
            return self
        T = torch.as_tensor(np.asarray(self.cam_T, dtype=np.float64), device=self.vertices.device)
        A, t = T[:3, :3], T[:3, 3]
        v = ((self.vertices.double() * float(self.scale)) @ A.t() + t).float()
        mirrored = float(np.linalg.det(np.asarray(self.cam_T, dtype=np.float64)[:3, :3])) < 0
        faces = self.faces[:, [0, 2, 1]].contiguous() if mirrored else self.faces
        nrm = None if self.normals is None else (self.normals.double() @ A.t()).float()
        out = Mesh(v, faces, nrm, scale=self.scale, cam_T=self.cam_T, sdf=self.sdf, frame="camera")
        out.lattice_vertices = self.vertices                   # the vertex order is kept: the NOCS attributes of the camera-frame mesh
        return out

    def signed_distance(self, points, want_sign=True):
        """float32 [n] on the device: the signed distance of points [n][3] (device tensor, this mesh's frame) to this mesh; negative inside.
        The one-mesh form of sdf_samples.mesh_sdf_many (`.sdf` is taken: it holds the lattice samples)."""
        from .sdf_samples import mesh_sdf_many
        return mesh_sdf_many([self], [points], want_sign=want_sign).sdf

    def encode(self, dsdf, n=500000, generator=None, **kw):
        """the latent of this (lattice-frame) mesh under the frozen decoder dsdf: encode.encode_meshes on this one mesh -> Encoded"""
        from .encode import encode_meshes
        return encode_meshes(dsdf, [self], n=n, generator=generator, **kw)

    def save(self, path, drop_degenerate=False):
        """binary little-endian PLY (with normals when the mesh has them) or OBJ, by extension.  Host code."""
        v, n, f = self.vertices_numpy(), self.normals_numpy(), self.faces_numpy(drop_degenerate)
        p = str(path)
        if p.lower().endswith(".ply"):
            _save_ply(p, v, n, f)
        elif p.lower().endswith(".obj"):
            _save_obj(p, v, n, f)
        else:
            raise ValueError("Mesh.save: the extension must be .ply or .obj")


def _areas(v, f):
    v = np.asarray(v, dtype=np.float64)
    return 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)


def _save_ply(path, v, n, f):
    props = "property float x\nproperty float y\nproperty float z\n"
    if n is not None:
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    head = ("ply\nformat binary_little_endian 1.0\ncomment sdflabel_amd mesh\nelement vertex %d\n%selement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % (len(v), props, len(f)))
    vert = np.asarray(v, dtype="<f4") if n is None else np.concatenate([np.asarray(v, "<f4"), np.asarray(n, "<f4")], 1)
    rec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    rec["n"], rec["i"] = 3, f
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(np.ascontiguousarray(vert, dtype="<f4").tobytes())
        fh.write(rec.tobytes())


def _save_obj(path, v, n, f):
    with open(path, "w") as fh:
        fh.write("# sdflabel_amd mesh\n")
        for p in v:
            fh.write("v %.9g %.9g %.9g\n" % tuple(float(x) for x in p))
        if n is not None:
            for p in n:
                fh.write("vn %.9g %.9g %.9g\n" % tuple(float(x) for x in p))
        for t in np.asarray(f) + 1:
            fh.write(("f %d//%d %d//%d %d//%d\n" % (t[0], t[0], t[1], t[1], t[2], t[2])) if n is not None else ("f %d %d %d\n" % tuple(t)))


def load_ply(path):
    """(vertices float32 [V][3], normals float32 [V][3] or None, faces int32 [T][3]) of a binary little-endian PLY as Mesh.save writes it"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or "format binary_little_endian 1.0" not in lines:
        raise ValueError("load_ply: not a binary little-endian PLY")
    nv = nf = 0
    props, elem = [], None
    for ln in lines:
        w = ln.split()
        if w[:1] == ["element"]:
            elem = w[1]
            if elem == "vertex":
                nv = int(w[2])
            elif elem == "face":
                nf = int(w[2])
        elif w[:1] == ["property"] and elem == "vertex":
            if w[1] != "float":
                raise ValueError("load_ply: vertex properties must be float")
            props.append(w[2])
    k = len(props)
    vert = np.frombuffer(data, dtype="<f4", count=nv * k, offset=end).reshape(nv, k)
    rec = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nf, offset=end + 4 * nv * k)
    if nf and (rec["n"] != 3).any():
        raise ValueError("load_ply: triangles only")
    v = np.ascontiguousarray(vert[:, [props.index(c) for c in "xyz"]], dtype=np.float32)
    n = np.ascontiguousarray(vert[:, [props.index(c) for c in ("nx", "ny", "nz")]], dtype=np.float32) if "nx" in props else None
    return v, n, np.ascontiguousarray(rec["i"], dtype=np.int32)


def load_obj(path):
    """(vertices float32 [V][3], normals float32 [V][3] or None, faces int32 [T][3]) of a Wavefront OBJ: `v` and `f` lines (and `vn`), polygons
    fanned from their first vertex, indices 1-based or negative (relative to the vertices read so far), `a/b/c` forms accepted.  The normals
    are returned only when there is one per vertex and every corner names the same index for both, as Mesh.save writes them."""
    v, vn, faces = [], [], []
    per_vertex = True
    with open(path, "r") as fh:
        for ln in fh:
            w = ln.split("#")[0].split()
            if not w:
                continue
            if w[0] == "v":
                v.append([float(x) for x in w[1:4]])
            elif w[0] == "vn":
                vn.append([float(x) for x in w[1:4]])
            elif w[0] == "f":
                idx = []
                for c in w[1:]:
                    parts = c.split("/")
                    i = int(parts[0])
                    i = i - 1 if i > 0 else len(v) + i
                    if not 0 <= i < len(v):
                        raise ValueError("load_obj: face index %s outside the %d vertices read so far" % (parts[0], len(v)))
                    if len(parts) == 3 and parts[2]:
                        k = int(parts[2])
                        per_vertex &= (k - 1 if k > 0 else len(vn) + k) == i
                    else:
                        per_vertex = False
                    idx.append(i)
                if len(idx) < 3:
                    raise ValueError("load_obj: a face with fewer than three vertices")
                faces += [(idx[0], idx[k], idx[k + 1]) for k in range(1, len(idx) - 1)]
    vert = np.asarray(v, dtype=np.float32).reshape(-1, 3)
    nrm = np.asarray(vn, dtype=np.float32).reshape(-1, 3) if per_vertex and vn and len(vn) == len(v) else None
    return vert, nrm, np.asarray(faces, dtype=np.int32).reshape(-1, 3)


# ---- extraction ----------------------------------------------------------------------------------------------------------------------------

def _check_R(R):
    if not (R_MIN <= int(R) <= R_MAX):
        raise ValueError("mesh: the lattice resolution must be %d .. %d (got %r)" % (R_MIN, R_MAX, R))


def _extract(sdf, R, B):
    """sdf: float32 [B * R^3] on the device.  Count, one host read of the totals, exact allocation, emit.  Returns (vertices [V][3],
    faces [T][3], voff, toff) with the host offsets of the shapes."""
    L = _lib.lib()
    dev = sdf.device
    nbytes = int(L.sdfr_mesh_ws_bytes(R, B))
    if nbytes < 0:
        raise _lib.SdfrError("mesh: B * R^3 must stay below 2^31 (B = %d, R = %d)" % (B, R))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    counts = torch.empty((2, B), dtype=torch.int32, device=dev)
    with _lib.guard(dev):
        st = _lib.stream_ptr()
        _lib.check(L.sdfr_mesh_count(_lib.ptr(sdf), R, B, _lib.ptr(counts[0]), _lib.ptr(counts[1]), _lib.ptr(ws), nbytes, st), "sdfr_mesh_count")
        host = counts.cpu().numpy().astype(np.int64)                     # the only host synchronisation
        voff = np.concatenate([[0], np.cumsum(host[0])]).astype(np.int64)
        toff = np.concatenate([[0], np.cumsum(host[1])]).astype(np.int64)
        V, T = int(voff[-1]), int(toff[-1])
        verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((T, 3), dtype=torch.int32, device=dev)
        _lib.check(L.sdfr_mesh_emit(_lib.ptr(sdf), R, B, voff.ctypes.data, toff.ctypes.data, _lib.ptr(ws), nbytes, _lib.ptr(verts) if V else None,
                                    V, _lib.ptr(faces) if T else None, T, st), "sdfr_mesh_emit")
    return verts, faces, voff, toff


@_lib.traced("mesh_from_sdf")
def mesh_from_sdf(sdf):
    """The iso-surface of SDF samples on the lattice: sdf float32 [B][R][R][R] or [R][R][R] on the GPU -> a list of B Mesh (vertices in the
    lattice frame, no normals).  Inside is sdf < 0; an exact 0 and a NaN are outside.  One host synchronisation."""
    if not torch.is_tensor(sdf) or not sdf.is_cuda:
        raise _lib.SdfrError("mesh_from_sdf runs on the GPU only; there is no CPU fallback")
    if sdf.dim() == 3:
        sdf = sdf[None]
    if sdf.dim() != 4 or not (sdf.shape[1] == sdf.shape[2] == sdf.shape[3]):
        raise ValueError("mesh_from_sdf: sdf must be [B][R][R][R] or [R][R][R]")
    B, R = int(sdf.shape[0]), int(sdf.shape[1])
    _check_R(R)
    if B == 0:
        return []
    flat = sdf.detach().float().contiguous().view(-1)
    verts, faces, voff, toff = _extract(flat, R, B)
    return [Mesh(verts[voff[b]:voff[b + 1]], faces[toff[b]:toff[b + 1]]) for b in range(B)]


def _latent_rows(shapes, device):
    """([B][L] float32 latents, per shape (scale, yaw, trans) or None) of a list of parameter dicts, a list of latents or a [B][L] tensor"""
    if torch.is_tensor(shapes):
        return shapes.detach().to(device).float().reshape(shapes.shape[0], -1).contiguous(), [None] * int(shapes.shape[0])
    lats, extra = [], []
    for p in shapes:
        if isinstance(p, dict):
            lats.append(torch.as_tensor(p["latent"]).detach().to(device).float().reshape(-1))
            extra.append(p if all(k in p for k in ("scale", "yaw", "trans")) else None)
        else:
            lats.append(torch.as_tensor(p).detach().to(device).float().reshape(-1))
            extra.append(None)
    return (torch.stack(lats).contiguous() if lats else torch.zeros((0, 0), device=device)), extra


def _host(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _decoder_mode(dsdf, device):
    handle = dsdf.handle(device)
    mp = getattr(dsdf, "mlp_precision", torch.float32)
    f16 = mp == torch.float16 and not handle.has_ln
    split = mp == "float32_split" and not handle.has_ln and handle.hp == 512
    L = _lib.lib()
    fwd = L.sdfr_mlp_forward_f16 if f16 else (L.sdfr_mlp_forward_split if split else L.sdfr_mlp_forward)
    return handle, fwd, f16


def lattice_sdf(dsdf, latents, R, staging_bytes=STAGING_BYTES):
    """The decoder on the lattice for latents [B][L] (raw, as given): float32 [B][R^3].  The input rows are staged in chunks of at most
    staging_bytes -- whole shapes while they fit, row ranges (multiples of 128 rows) of one shape otherwise; every row gets the value it gets
    in a single launch."""
    L = _lib.lib()
    dev = latents.device
    handle, fwd, _ = _decoder_mode(dsdf, dev)
    B, Ld = int(latents.shape[0]), int(latents.shape[1])
    if Ld != int(dsdf.latent_size):
        raise ValueError("mesh: latents of size %d for a decoder of latent size %d" % (Ld, dsdf.latent_size))
    NI, G = Ld + 3, R ** 3
    budget = max(128, int(staging_bytes) // (4 * NI) // 128 * 128)                 # rows in flight
    sdf = torch.empty((B, G), dtype=torch.float32, device=dev)
    P, ck = _lib.ptr, _lib.check
    with _lib.guard(dev):
        st = _lib.stream_ptr()
        if G <= budget:
            nb = max(1, budget // G)
            inputs = torch.empty((min(nb, B) * G, NI), dtype=torch.float32, device=dev)
            for b0 in range(0, B, nb):
                n = min(nb, B - b0)
                ck(L.sdfr_mesh_lattice_inputs(P(latents[b0:]), Ld, R, n, 0, G, P(inputs), st), "sdfr_mesh_lattice_inputs")
                ck(fwd(handle.h, P(inputs), n * G, P(sdf[b0:]), None, st), fwd.__name__)
        else:
            inputs = torch.empty((budget, NI), dtype=torch.float32, device=dev)
            for b in range(B):
                for r0 in range(0, G, budget):
                    n = min(budget, G - r0)
                    ck(L.sdfr_mesh_lattice_inputs(P(latents[b:]), Ld, R, 1, r0, n, P(inputs), st), "sdfr_mesh_lattice_inputs")
                    ck(fwd(handle.h, P(inputs), n, P(sdf[b, r0:]), None, st), fwd.__name__)
    return sdf


def decoder_rows(handle, fwd, f16, inputs, n, sdf, J, sel, masks, idx, cnt, st):
    """One staged chunk of n decoder rows: the forward `fwd` of _decoder_mode (masks saved) and sdfr_mlp_jacobian with the identity index list
    idx [n] / cnt [1] = n, into sdf [n], J [n][n_inputs] and sel [n].  The two launches decoder_at makes per chunk and encode.encode_many makes
    per iteration.  masks is None for LayerNorm decoders: they save none, and their Jacobian recomputes the forward."""
    L = _lib.lib()
    P, ck = _lib.ptr, _lib.check
    ck(fwd(handle.h, P(inputs), n, P(sdf), P(masks), st), fwd.__name__)
    ck(L.sdfr_mlp_jacobian(handle.h, P(inputs), n, 1, P(idx), n, P(cnt), P(J), P(sel), P(sdf) if masks is not None else None, P(masks),
                           2 if f16 else 0, st), "sdfr_mlp_jacobian")


def decoder_at(dsdf, latents, shape_of, points, staging_bytes=STAGING_BYTES):
    """The decoder, its Jacobian and the Newton projection at `points` [n][3] of the shapes shape_of [n] (int64 rows of latents): the calls
    Grid3D.get_surface_points makes for its band, with an identity index list.  Returns (projected points p - sdf n, unit normals n, sdf)."""
    L = _lib.lib()
    dev = points.device
    handle, fwd, f16 = _decoder_mode(dsdf, dev)
    Ld = int(latents.shape[1])
    NI, n_all = Ld + 3, int(points.shape[0])
    budget = max(128, int(staging_bytes) // (4 * NI) // 128 * 128)
    proj = torch.empty((n_all, 3), dtype=torch.float32, device=dev)
    nrm = torch.empty((n_all, 3), dtype=torch.float32, device=dev)
    val = torch.empty((n_all,), dtype=torch.float32, device=dev)
    P, ck = _lib.ptr, _lib.check
    with _lib.guard(dev):
        st = _lib.stream_ptr()
        for r0 in range(0, n_all, budget):
            n = min(budget, n_all - r0)
            inputs = torch.cat([latents.index_select(0, shape_of[r0:r0 + n]), points[r0:r0 + n]], 1).contiguous()
            idx = torch.arange(n, dtype=torch.int32, device=dev)
            cnt = torch.full((1,), n, dtype=torch.int32, device=dev)
            J = torch.empty((n, NI), dtype=torch.float32, device=dev)
            sel = torch.empty((n,), dtype=torch.float32, device=dev)
            sdf = val[r0:r0 + n]
            masks = None if handle.has_ln else torch.empty((int(L.sdfr_decoder_mask_words(handle.h, n)),), dtype=torch.int32, device=dev)
            decoder_rows(handle, fwd, f16, inputs, n, sdf, J, sel, masks, idx, cnt, st)
            ck(L.sdfr_surface_project(P(inputs[:, Ld:]), NI, P(sdf), n, 1, P(idx), n, P(cnt), P(J), NI, Ld, P(proj[r0:]), None, P(nrm[r0:]), st),
               "sdfr_surface_project")
    return proj, nrm, val


@_lib.traced("meshes_many")
def meshes_many(dsdf, shapes, resolution=64, polish=True, normals=True, return_sdf=False, max_batch=16, staging_bytes=STAGING_BYTES):
    """Triangle meshes of DeepSDF shapes.

    shapes: a list of parameter dicts {'latent', and optionally 'scale', 'yaw', 'trans'} as Optimizer.optimize_many leaves them, a list of
    latents, or a [B][L] tensor.  THE LATENT GOES TO THE DECODER RAW, as labels_many and get_kitti_label pass it: the mesh is the shape the
    label was computed from.  The decoder's mlp_precision picks the forward kernel.
    resolution: lattice points per axis (2 .. 256).  polish: move every vertex by p - sdf(p) n(p) with the decoder's own value and normal at
    the vertex (one Newton step; the welded topology is unchanged).  normals: keep the decoder's unit normals at the vertices (with
    polish=False they come from the same Jacobian, evaluated at the unpolished vertices).  return_sdf: keep the [R][R][R] samples on each
    mesh.  Per chunk of max_batch shapes: the decoder over the lattice, count, ONE host read of the totals, emit, polish.
    With 'scale', 'yaw' and 'trans' present a mesh carries .scale and .cam_T (frame.assemble_labels' matrix) for to_camera().
    Returns a list of Mesh in the lattice frame; a shape without a sign change gives an empty mesh."""
    R = int(resolution)
    _check_R(R)
    dev = next(dsdf.parameters()).device
    if dev.type != "cuda":
        raise _lib.SdfrError("meshes_many runs on the GPU only; there is no CPU fallback")
    latents, extra = _latent_rows(shapes, dev)
    out = []
    step = max(1, int(max_batch))
    for c0 in range(0, int(latents.shape[0]), step):
        lat = latents[c0:c0 + step].contiguous()
        B = int(lat.shape[0])
        sdf = lattice_sdf(dsdf, lat, R, staging_bytes)
        verts, faces, voff, toff = _extract(sdf.view(-1), R, B)
        nrm = None
        if (polish or normals) and verts.shape[0] > 0:
            shape_of = torch.repeat_interleave(torch.arange(B, device=dev), torch.as_tensor(np.diff(voff), device=dev))
            proj, nrm, _ = decoder_at(dsdf, lat, shape_of, verts, staging_bytes)
            if polish:
                verts = proj
            if not normals:
                nrm = None
        elif normals:
            nrm = torch.empty((0, 3), dtype=torch.float32, device=dev)
        for b in range(B):
            m = Mesh(verts[voff[b]:voff[b + 1]], faces[toff[b]:toff[b + 1]], None if nrm is None else nrm[voff[b]:voff[b + 1]],
                     sdf=sdf[b].view(R, R, R) if return_sdf else None)
            p = extra[c0 + b]
            if p is not None:
                from .frame import assemble_labels
                scale = np.asarray(_host(p["scale"]), dtype=np.float32).reshape(-1)[:1]
                _, cam_T = assemble_labels(np.zeros((1, 6), np.float32), np.asarray(_host(p["yaw"]), np.float32).reshape(-1)[:1],
                                           np.asarray(_host(p["trans"]), np.float32).reshape(1, 3), scale, np.eye(4), [None])
                m.scale, m.cam_T = float(scale[0]), cam_T[0]
            out.append(m)
    return out
