"""Signed distances to triangle meshes and the sample sets a DeepSDF prior is trained on (csrc/mesh_sdf.hip; DESIGN.md "Signed distances to
meshes").

    from sdflabel_amd.sdf_samples import mesh_sdf_many, surface_points_many, fit_frame, normalize, draw_sdf_samples, SdfSamples, prior_residuals

mesh_sdf_many        how far is each query point from its mesh, and on which side: exact, all pairs, float64
surface_points_many  area-weighted points on the meshes from uniforms drawn on the host
fit_frame, normalize centre and scale that bring a CAD model into the lattice frame
draw_sdf_samples     near-surface and uniform samples with their signed distances: SdfSamples, saved as DeepSDF's .npz layout
prior_residuals      how well a decoder and a latent explain such samples: the quantity training a prior minimises

Everything packs its inputs once and launches without waiting for the device; the only host read is SdfSamples.save / .numpy.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .pose import _upload

MeshSdf = namedtuple("MeshSdf", "sdf nearest winding flags offsets")
MeshSdf.__doc__ = """sdf float32 [N], nearest int32 [N] or None, winding float64 [N] or None, flags int32 [B]: device tensors; offsets: host int64
[B + 1], the meshes' runs in the point arrays"""


def _mesh_arrays(m):
    v, f = (m.vertices, m.faces) if hasattr(m, "vertices") else m
    return torch.as_tensor(v), torch.as_tensor(f)


class MeshBatch:
    """B meshes packed once: `.vertices` float32 [V][3], `.faces` int32 [T][3], `.d_voff` / `.d_toff` int64 [B + 1] on the device and
    `.voff` / `.toff` on the host.  Takes Mesh objects or (vertices, faces) pairs of device tensors."""

    def __init__(self, meshes):
        pairs = [_mesh_arrays(m) for m in meshes]
        for v, f in pairs:
            if not (v.is_cuda and f.is_cuda):
                raise _lib.SdfrError("mesh_sdf runs on the GPU only; there is no CPU fallback")
        self.B = len(pairs)
        if self.B == 0:
            raise ValueError("mesh_sdf: no meshes")
        self.device = pairs[0][0].device
        self.voff = np.concatenate([[0], np.cumsum([int(v.shape[0]) for v, _ in pairs])]).astype(np.int64)
        self.toff = np.concatenate([[0], np.cumsum([int(f.shape[0]) for _, f in pairs])]).astype(np.int64)
        self.vertices = torch.cat([v.detach().float().reshape(-1, 3) for v, _ in pairs]).contiguous()
        self.faces = torch.cat([f.detach().to(torch.int32).reshape(-1, 3) for _, f in pairs]).contiguous()
        table = _upload(torch.from_numpy(np.concatenate([self.voff, self.toff])), self.device)
        self.d_voff, self.d_toff = table[:self.B + 1], table[self.B + 1:]
        self.V, self.T = int(self.voff[-1]), int(self.toff[-1])


def _batch(meshes):
    return meshes if isinstance(meshes, MeshBatch) else MeshBatch(list(meshes))


def _ragged(points, offsets, B, device):
    """points: one [N][3] tensor with host offsets [B + 1], or a list of B tensors [n_i][3] -> (float32 [N][3] on the device, host offsets)"""
    if torch.is_tensor(points):
        if offsets is None:
            if B != 1:
                raise ValueError("mesh_sdf: one point tensor for %d meshes needs offsets" % B)
            offsets = [0, int(points.shape[0])]
        pts = points
    else:
        points = list(points)
        if offsets is not None:
            raise ValueError("mesh_sdf: offsets go with one packed point tensor, not with a list")
        offsets = np.concatenate([[0], np.cumsum([int(p.shape[0]) for p in points])])
        pts = torch.cat([p.reshape(-1, 3) for p in points]) if points else torch.zeros((0, 3), device=device)
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if not pts.is_cuda:
        raise _lib.SdfrError("mesh_sdf runs on the GPU only; there is no CPU fallback")
    pts = pts.detach().float().reshape(-1, 3).contiguous()
    if len(off) != B + 1 or off[0] != 0 or off[-1] != pts.shape[0] or (np.diff(off) < 0).any():
        raise ValueError("mesh_sdf: offsets must rise from 0 to the number of points, one run per mesh")
    return pts, off


@_lib.traced("mesh_sdf_many")
def mesh_sdf_many(meshes, points, offsets=None, want_sign=True, return_nearest=False, return_winding=False):
    """The signed distance of every query point to its mesh.

    meshes: Mesh objects, (vertices, faces) pairs, or a MeshBatch.  points: a list with one [n_i][3] tensor per mesh, or one packed [N][3]
    tensor with `offsets` (host integers, [B + 1]).  want_sign=False gives the unsigned distance and skips the winding pass: for open meshes.
    Inside is |winding number| >= 0.5, so outward- and inward-wound meshes (Mesh.to_camera reverses the winding) both work; zero-area
    triangles act as segments or points; triangles with non-finite vertices or indices outside the mesh are skipped and reported in the
    flags (bit 0, bit 1).  A non-finite point and a point of a mesh without a usable triangle get +inf.
    Returns MeshSdf(sdf, nearest, winding, flags, offsets): device tensors, nothing is read back."""
    L = _lib.lib()
    mb = _batch(meshes)
    dev = mb.device
    pts, off = _ragged(points, offsets, mb.B, dev)
    N = int(pts.shape[0])
    d_qoff = _upload(torch.from_numpy(off), dev)
    nbytes = int(L.sdfr_mesh_sdf_ws_bytes(mb.B, N, mb.T))
    if nbytes < 0:
        raise _lib.SdfrError("mesh_sdf: sizes out of range (B = %d, N = %d, T = %d)" % (mb.B, N, mb.T))
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
    sdf = torch.empty((N,), dtype=torch.float32, device=dev)
    nearest = torch.empty((N,), dtype=torch.int32, device=dev) if return_nearest else None
    winding = torch.empty((N,), dtype=torch.float64, device=dev) if return_winding else None
    flags = torch.empty((mb.B,), dtype=torch.int32, device=dev)
    P = _lib.ptr
    with _lib.guard(dev):
        _lib.check(L.sdfr_mesh_sdf(P(mb.vertices) if mb.V else None, mb.V, P(mb.faces) if mb.T else None, mb.T, P(mb.d_voff), P(mb.d_toff),
                                   P(pts) if N else None, N, P(d_qoff), mb.B, 1 if want_sign else 0, P(ws), nbytes, P(sdf) if N else None, None,
                                   None, P(nearest) if N else None, P(winding) if N else None, P(flags), _lib.stream_ptr()), "sdfr_mesh_sdf")
    return MeshSdf(sdf, nearest, winding, flags, off)


@_lib.traced("surface_points_many")
def surface_points_many(meshes, counts, generator):
    """Area-weighted random points on the meshes.  counts: samples per mesh (host integers); generator: the caller's torch.Generator on the
    HOST, from which 3 uniforms per sample are drawn in mesh order.  Returns (points float32 [S][3], triangle int32 [S], flags int32 [B],
    offsets host int64 [B + 1]); a mesh without area gives triangle = -1, zero points and flag bit 1."""
    L = _lib.lib()
    mb = _batch(meshes)
    dev = mb.device
    counts = [int(c) for c in (counts if hasattr(counts, "__len__") else [counts] * mb.B)]
    if len(counts) != mb.B or min(counts) < 0:
        raise ValueError("surface_points_many: one non-negative count per mesh")
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    S = int(off[-1])
    u = _upload(torch.rand((S, 3), generator=generator, dtype=torch.float32), dev)
    return _surface_points(L, mb, u, off)


def _surface_points(L, mb, u, off):
    dev = mb.device
    S = int(u.shape[0])
    d_soff = _upload(torch.from_numpy(off), dev)
    nbytes = int(L.sdfr_mesh_surface_ws_bytes(mb.B, mb.T))
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
    pts = torch.empty((S, 3), dtype=torch.float32, device=dev)
    tri = torch.empty((S,), dtype=torch.int32, device=dev)
    flags = torch.empty((mb.B,), dtype=torch.int32, device=dev)
    P = _lib.ptr
    with _lib.guard(dev):
        _lib.check(L.sdfr_mesh_surface_points(P(mb.vertices) if mb.V else None, mb.V, P(mb.faces) if mb.T else None, mb.T, P(mb.d_voff),
                                              P(mb.d_toff), P(u) if S else None, S, P(d_soff), mb.B, P(ws), nbytes, P(pts) if S else None,
                                              P(tri) if S else None, P(flags), _lib.stream_ptr()), "sdfr_mesh_surface_points")
    return pts, tri, flags, off


def fit_frame(vertices, mode="unit_sphere", buffer=1.03):
    """(centre float64 [3], scale float64) that bring a model into the lattice frame: x -> (x - centre) * scale.  The centre is the middle of
    the bounding box.  'unit_sphere': the farthest vertex lands at radius 1 / buffer (DeepSDF's normalisation as recalled); 'unit_cube': the
    longest half extent lands at 1 / buffer; None: the identity.  Host code, float64."""
    if mode is None:
        return np.zeros(3), 1.0
    v = (vertices.detach().cpu().numpy() if torch.is_tensor(vertices) else np.asarray(vertices)).astype(np.float64).reshape(-1, 3)
    v = v[np.isfinite(v).all(1)]
    if len(v) == 0:
        raise ValueError("fit_frame: no finite vertex")
    lo, hi = v.min(0), v.max(0)
    centre = (lo + hi) / 2.0
    if mode == "unit_sphere":
        size = float(np.sqrt(((v - centre) ** 2).sum(1)).max())
    elif mode == "unit_cube":
        size = float(((hi - lo) / 2.0).max())
    else:
        raise ValueError("fit_frame: mode must be 'unit_sphere', 'unit_cube' or None (got %r)" % (mode,))
    if not size > 0:
        raise ValueError("fit_frame: the model has no extent")
    return centre, 1.0 / (size * float(buffer))


def normalize(vertices, centre, scale):
    """(vertices - centre) * scale in float64, rounded once to float32; a tensor stays on its device, an array stays an array"""
    if torch.is_tensor(vertices):
        c = torch.as_tensor(np.asarray(centre, np.float64), device=vertices.device)
        return ((vertices.double() - c) * float(scale)).float()
    return ((np.asarray(vertices, np.float64) - np.asarray(centre, np.float64)) * float(scale)).astype(np.float32)


class SdfSamples:
    """The training samples of one shape: `.rows` float32 [n][4] = x y z sdf (a device tensor after draw_sdf_samples, a host tensor after
    load), `.flags` the mesh's flag word (a 0-d tensor, or None after load), `.counts` = (near with the first width, near with the second,
    uniform)."""

    def __init__(self, rows, flags=None, counts=None):
        self.rows, self.flags, self.counts = rows, flags, counts

    def __len__(self):
        return int(self.rows.shape[0])

    def numpy(self):
        return self.rows.detach().cpu().numpy()

    def save(self, path):
        """DeepSDF's .npz layout: `pos` float32 [k][4] the rows with sdf >= 0 and `neg` the rows with sdf < 0, each in the order drawn.  One
        host read."""
        r = self.numpy()
        neg = r[:, 3] < 0
        np.savez(path, pos=np.ascontiguousarray(r[~neg]), neg=np.ascontiguousarray(r[neg]))

    @staticmethod
    def load(path, device=None):
        z = np.load(path)
        rows = torch.from_numpy(np.concatenate([np.asarray(z["pos"], np.float32).reshape(-1, 4), np.asarray(z["neg"], np.float32).reshape(-1, 4)]))
        return SdfSamples(rows if device is None else rows.to(device), None, None)


def sample_counts(n, near_share):
    """(near with the first width, near with the second, uniform) for n samples"""
    a, b = int(round(n * float(near_share[0]))), int(round(n * float(near_share[1])))
    if min(a, b) < 0 or a + b > n:
        raise ValueError("draw_sdf_samples: near_share must be two non-negative shares that sum to at most 1")
    return a, b, n - a - b


@_lib.traced("draw_sdf_samples")
def draw_sdf_samples(meshes, n=500000, generator=None, near_share=(0.47, 0.47), sigmas=(0.005 ** 0.5, 0.0005 ** 0.5), half_extent=1.0,
                     want_sign=True):
    """Samples x y z sdf of every mesh, as a DeepSDF decoder is trained on them: per mesh n near_share[0] surface points perturbed by a
    Gaussian of width sigmas[0], n near_share[1] by sigmas[1], and the rest uniform in the cube [-half_extent, half_extent]^3; all signed
    with mesh_sdf_many.  The meshes should be in the lattice frame (fit_frame / normalize).

    THE DEFAULTS ARE DeepSDF's AS RECALLED -- 500 000 samples, 47 % / 47 % / 6 %, variances 0.005 and 0.0005 in the unit sphere.  They are
    parameters; they have not been checked against that paper's code.

    generator: a torch.Generator on the HOST (as synth.draw_scenes and augment.draw_params take theirs); everything random is drawn from it in
    a fixed order: the sampler's uniforms of all meshes, then per mesh the Gaussian offsets and the cube's uniforms.  Nothing is read back from
    the device.  Returns a list of SdfSamples, rows ordered near (first width), near (second width), uniform."""
    L = _lib.lib()
    mb = _batch(meshes)
    dev = mb.device
    if generator is None:
        raise ValueError("draw_sdf_samples: pass a torch.Generator (host) -- the draw must be repeatable")
    na, nb, nu = sample_counts(int(n), near_share)
    off = np.arange(mb.B + 1, dtype=np.int64) * (na + nb)
    u = _upload(torch.rand((int(off[-1]), 3), generator=generator, dtype=torch.float32), dev)
    surf, _, _, _ = _surface_points(L, mb, u, off)
    width = torch.cat([torch.full((na, 1), float(sigmas[0])), torch.full((nb, 1), float(sigmas[1]))])
    pts = []
    for b in range(mb.B):
        noise = _upload(torch.randn((na + nb, 3), generator=generator, dtype=torch.float32) * width, dev)
        cube = _upload((torch.rand((nu, 3), generator=generator, dtype=torch.float32) * 2.0 - 1.0) * float(half_extent), dev)
        pts.append(torch.cat([surf[off[b]:off[b + 1]] + noise, cube]))
    res = mesh_sdf_many(mb, pts, want_sign=want_sign)
    rows = torch.cat([torch.cat(pts), res.sdf[:, None]], 1)
    return [SdfSamples(rows[b * int(n):(b + 1) * int(n)], res.flags[b], (na, nb, nu)) for b in range(mb.B)]


@_lib.traced("prior_residuals")
def prior_residuals(dsdf, latents, samples, clamp=0.1):
    """How well the decoder `dsdf` with latents [B][L] (raw, as meshes_many takes them) explains the samples (a list of B SdfSamples, or one):
    per shape the mean of |clamp(decoder) - clamp(sdf)| with both clamped to [-clamp, clamp] -- DeepSDF's training loss without its latent
    regulariser -- and the share of samples whose sign agrees (sdf < 0 on both sides or on neither).  The decoder is evaluated through
    mesh.decoder_at.  Returns (l1 float64 [B], sign_agreement float64 [B]) on the device; rows with a non-finite sdf are left out."""
    from .mesh import decoder_at
    samples = [samples] if isinstance(samples, SdfSamples) else list(samples)
    dev = next(dsdf.parameters()).device
    lat = torch.as_tensor(latents).detach().to(dev).float().reshape(len(samples), -1).contiguous()
    rows = torch.cat([s.rows.to(dev) for s in samples]).float().contiguous()
    counts = [len(s) for s in samples]
    shape_of = torch.repeat_interleave(torch.arange(len(samples), device=dev), _upload(torch.tensor(counts, dtype=torch.int64), dev),
                                       output_size=int(sum(counts)))
    _, _, val = decoder_at(dsdf, lat, shape_of, rows[:, :3].contiguous())
    want = rows[:, 3]
    ok = torch.isfinite(want) & torch.isfinite(val)
    c = float(clamp)
    err = torch.where(ok, (val.clamp(-c, c) - want.clamp(-c, c)).abs().double(), torch.zeros((), dtype=torch.float64, device=dev))
    agree = torch.where(ok, ((val < 0) == (want < 0)).double(), torch.zeros((), dtype=torch.float64, device=dev))
    zero = torch.zeros((len(samples),), dtype=torch.float64, device=dev)
    cnt = zero.index_add(0, shape_of, ok.double()).clamp(min=1.0)
    return zero.index_add(0, shape_of, err) / cnt, zero.index_add(0, shape_of, agree) / cnt
