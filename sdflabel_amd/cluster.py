"""Object proposals from a raw scan on the device: lidar clusters and rough boxes (csrc/cluster.hip).

    from sdflabel_amd.cluster import clusters, boxes, proposals

align.align_many fits yaw, trans and latent to a lidar cloud "from any rough box".  This module makes that rough box without 2-D
annotations and without a CSS network: Euclidean clustering of the (road-free) cloud -- which points belong together --, and per cluster the
minimum-area rectangle in the camera's x-z plane over a table of directions, with the y extent -- where the object is, roughly, and which
way it lies.  The reference has no counterpart to this stage; the semantics are this project's own and are pinned by the numpy restatement
tests/_cluster_ref.py.

  clusters    sdfr_lidar_clusters: label per point, member lists in ascending input index, offsets, counts.  No host synchronisation.
  boxes       sdfr_cluster_boxes: the rectangle of every kept cluster.  No host synchronisation.
  proposals   both, ONE host read (counts, offsets, rectangles), the gates, and per accepted cluster the start {'yaw', 'trans', 'scale',
              'latent'} for align_many, its cloud and an info dict.  Front and back cannot be told apart from a rectangle: every cluster
              yields the hypotheses yaw and yaw + pi.

THE DEFAULTS (eps = 0.5 m, min_points = 10, no upper gate on the size, 512 clusters, 90 directions over a quarter turn, scale = 2.0, the
gates on length, width and height) ARE PARAMETERS WITHOUT A CLAIMED OPERATING POINT.  They are round numbers that separate car-sized objects
in the synthetic scenes of the tests; nothing is claimed of them on real scans.

Out of scope: core-point (DBSCAN) filtering; class-prior box sizes anchored at the near corner; several scans per call; telling front from
back other than by the fit's loss (pipelines.scan.label_scan); any claim about label quality on real scans.
"""
import math

import numpy as np
import torch

from . import _lib
from .frame import _cloud, _device
from .pose import _as_tensor, _upload

P, ck = _lib.ptr, _lib.check
CAPPED, NONFINITE = 1, 2                                                 # Clusters.counts[3] (csrc/cluster_cells.h)
MAX_CLUSTERS, MAX_DIRS = 4096, 1024
GATES = {"length": (1.0, 8.0), "width": (0.5, 3.5), "height": (0.5, 3.5)}


class Clusters:
    """`.label` int32 [N]: the cluster of every point, -1 for a point that takes no part, whose component is no cluster or whose cluster is
    beyond the cap.  `.members` int32 [N]: the input indices cluster by cluster, ascending within a cluster; the entries from
    offsets[kept] on are unspecified.  `.offsets` int32 [max_clusters + 1]; the entries beyond the kept count equal the total.  `.counts`
    int32 [4] = participating points, components, clusters found (capped or not), flags (1: the cap cut something, 2: a non-finite point
    under a set mask was left out).  `.points`: the cloud the indices refer to.  All on the device."""

    def __init__(self, label, members, offsets, counts, points, max_clusters):
        self.label, self.members, self.offsets, self.counts, self.points, self.max_clusters = label, members, offsets, counts, points, max_clusters


class Boxes:
    """`.rect` float64 [max_clusters][8] = k, u_min, u_max, v_min, v_max, y_min, y_max, area of each kept cluster's first direction of the
    smallest area (the rows beyond the kept count are unspecified); `.dirs` float64 [K][2] = (cos, sin) of the directions, as the kernel
    read them; `.dirs_host` the numpy array they were uploaded from."""

    def __init__(self, rect, dirs, dirs_host):
        self.rect, self.dirs, self.dirs_host = rect, dirs, dirs_host


def _check_clusters(eps, min_points, max_points, max_clusters):
    if not (float(eps) > 0 and math.isfinite(float(eps))):
        raise ValueError("clusters: eps must be positive and finite")
    if not 1 <= int(max_clusters) <= MAX_CLUSTERS:
        raise ValueError("clusters: max_clusters must be 1 ... %d" % MAX_CLUSTERS)
    return float(eps), int(min_points), 0 if max_points is None else int(max_points), int(max_clusters)


@_lib.traced("clusters")
def clusters(lidar, mask=None, eps=0.5, min_points=10, max_points=None, max_clusters=512, _out=None):
    """Euclidean clusters of a cloud.

    lidar [N][3], camera frame, float64 or float32 (widened first), host or device.  mask: None, or [N] -- frame.remove_road's `keep`;
    a point takes part if its mask is non-zero and its three coordinates are finite.  Two participating points are neighbours if
    d2 = (dx*dx + dy*dy) + dz*dz < eps*eps, strictly, in float64 (eps is rounded to float32 first; 0.5 is exact).  A connected component of
    that graph is a cluster if min_points <= size <= max_points (max_points None or <= 0: no upper gate).  Clusters are numbered in ascending
    order of their smallest member index; only the first max_clusters (at most 4096) are kept.  The same bits on every run.
    No host read and no host synchronisation.  Returns a Clusters."""
    eps, min_points, max_points, max_clusters = _check_clusters(eps, min_points, max_points, max_clusters)
    dev = _device(lidar, mask)
    if dev.type != "cuda":
        raise _lib.SdfrError("clusters runs on the GPU only; there is no CPU fallback")
    pts = _cloud(lidar, dev)
    N = int(pts.shape[0])
    m = None
    if mask is not None:
        m = _as_tensor(mask, dev).reshape(-1)
        if int(m.shape[0]) != N:
            raise ValueError("clusters: %d points, a mask of %d" % (N, int(m.shape[0])))
        m = (m.view(torch.uint8) if m.dtype == torch.bool else (m != 0).view(torch.uint8)).contiguous()
    L = _lib.lib()
    nbytes = int(L.sdfr_cluster_ws_bytes(N, max_clusters))
    if nbytes < 0:
        raise _lib.SdfrError("clusters: %d points with %d clusters are more than the library takes" % (N, max_clusters))
    i32 = dict(dtype=torch.int32, device=dev)
    if _out is None:
        label, members = torch.empty((N,), **i32), torch.empty((N,), **i32)
        off, counts = torch.empty((max_clusters + 1,), **i32), torch.empty((4,), **i32)
    else:                                                                # the tests' own buffers, between guard words
        label, members, off, counts = _out
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
    with _lib.guard(dev):
        ck(L.sdfr_lidar_clusters(P(pts), int(pts.dtype == torch.float64), N, P(m), eps, min_points, max_points, max_clusters, P(label), P(members),
                                 P(off), P(counts), P(ws), nbytes, _lib.stream_ptr()), "sdfr_lidar_clusters")
    return Clusters(label, members, off, counts, pts, max_clusters)


def directions(n_angles):
    """(cos, sin) float64 [n_angles][2] of theta_k = k (pi / 2) / n_angles, formed on the host with numpy: the range is [0, pi / 2) because a
    rectangle repeats after a quarter turn.  The kernel and the restatement read the same array, so no cosine has to agree within an ulp."""
    n = int(n_angles)
    if not 1 <= n <= MAX_DIRS:
        raise ValueError("boxes: n_angles must be 1 ... %d" % MAX_DIRS)
    th = np.arange(n, dtype=np.float64) * (np.pi / 2) / n
    return np.ascontiguousarray(np.stack([np.cos(th), np.sin(th)], 1))


@_lib.traced("boxes")
def boxes(lidar, clusters, n_angles=90, dirs=None, _out=None):
    """The minimum-area rectangle of every kept cluster in the camera's x-z plane over a table of directions, and its y extent.

    lidar: the cloud `clusters` was made from (None: clusters.points).  The directions are theta_k = k (pi / 2) / n_angles (`directions`),
    or the caller's table dirs [K][2] of (cos, sin), K <= 1024.  Per point and direction u = x c + z s, v = z c - x s in float64, every
    product and sum rounded once; per cluster and direction the extents of u and v and area = (u_max - u_min) (v_max - v_min); the winner
    is the first direction of the smallest area.  Only minima and maxima: the same bits on every run.
    No host read and no host synchronisation.  Returns a Boxes."""
    dirs_host = directions(n_angles) if dirs is None else np.ascontiguousarray(np.asarray(dirs, np.float64).reshape(-1, 2))
    K = int(dirs_host.shape[0])
    if not 1 <= K <= MAX_DIRS:
        raise ValueError("boxes: the direction table must hold 1 ... %d directions" % MAX_DIRS)
    pts = clusters.points if lidar is None else _cloud(lidar, clusters.label.device)
    dev = pts.device
    if dev.type != "cuda":
        raise _lib.SdfrError("boxes runs on the GPU only; there is no CPU fallback")
    N, C = int(pts.shape[0]), int(clusters.max_clusters)
    if N != int(clusters.label.shape[0]):
        raise ValueError("boxes: %d points, clusters of %d" % (N, int(clusters.label.shape[0])))
    d = _upload(torch.from_numpy(dirs_host), dev)
    rect = torch.empty((C, 8), dtype=torch.float64, device=dev) if _out is None else _out
    with _lib.guard(dev):
        ck(_lib.lib().sdfr_cluster_boxes(P(pts), int(pts.dtype == torch.float64), N, P(clusters.members), P(clusters.offsets), P(clusters.counts), C,
                                         P(d), K, P(rect), _lib.stream_ptr()), "sdfr_cluster_boxes")
    return Boxes(rect, d, dirs_host)


def starts_from_rect(rect, dirs, scale):
    """Host arithmetic, float64: rough poses from rectangles.  rect [A][8] and dirs [K][2] as `boxes` gives them, scale the lattice scale.

    The pose convention is verify_point_x64's: x = diag(1, -1, 1) rot(yaw)^T (p / scale - trans), i.e. x_2 = sin(yaw) q_0 + cos(yaw) q_2:
    in the camera's (x, z) the lattice z axis -- the length, as frame.assemble_labels takes dims = height, width, length from the y, x, z
    extents -- points along (sin yaw, cos yaw).  The rectangle's u axis is (cos th, sin th), its v axis (-sin th, cos th).  The longer
    side carries the length: u longer gives yaw = pi / 2 - th, otherwise (v longer, or a tie) yaw = -th.  The centre of the rectangle and
    of the y extent, divided by the scale, is trans.
    Returns (yaw [A], trans [A][3], dims [A][3] = length, width, height in metres)."""
    rect = np.asarray(rect, np.float64).reshape(-1, 8)
    dirs = np.asarray(dirs, np.float64).reshape(-1, 2)
    k = rect[:, 0].astype(np.int64)
    c, s = dirs[k, 0], dirs[k, 1]
    th = np.arctan2(s, c)
    du, dv = rect[:, 2] - rect[:, 1], rect[:, 4] - rect[:, 3]
    along_u = du > dv
    yaw = np.where(along_u, np.pi / 2 - th, -th)
    cu, cv, cy = (rect[:, 1] + rect[:, 2]) / 2, (rect[:, 3] + rect[:, 4]) / 2, (rect[:, 5] + rect[:, 6]) / 2
    centre = np.stack([cu * c - cv * s, cy, cu * s + cv * c], 1)
    dims = np.stack([np.maximum(du, dv), np.minimum(du, dv), rect[:, 6] - rect[:, 5]], 1)
    return yaw, centre / float(scale), dims


def _gate(gates):
    g = dict(GATES)
    if gates is not None:
        if any(k not in GATES for k in gates):
            raise ValueError("proposals: gates may hold 'length', 'width' and 'height' (got %r)" % (sorted(gates),))
        g.update({k: (float(v[0]), float(v[1])) for k, v in gates.items()})
    return np.array([g["length"], g["width"], g["height"]], np.float64)


class Proposals:
    """What `proposals` returns.  `.params[a]` and `.flipped[a]`: the two starts {'yaw' [1], 'trans' [3], 'scale' [1], 'latent' [L]} of
    accepted cluster a (yaw and yaw + pi), float32, in the shapes align_many takes.  `.clouds[a]`: its points float32 [n][3] on the device,
    a view of `.gathered` (all kept clusters' points in member order).  `.info[a]`: {'cluster', 'rect' (the 8 numbers), 'n', 'dims'
    (length, width, height, metres), 'yaw', 'centre'}.  `.clusters`, `.boxes`: the device results; `.counts`, `.offsets`, `.rect`: their host
    copies (numpy), `.kept` the number of kept clusters.  Iterating gives (params, cloud, info) per accepted cluster."""

    def __init__(self, params, flipped, clouds, info, gathered, clusters, boxes, counts, offsets, rect, kept):
        self.params, self.flipped, self.clouds, self.info, self.gathered = params, flipped, clouds, info, gathered
        self.clusters, self.boxes, self.counts, self.offsets, self.rect, self.kept = clusters, boxes, counts, offsets, rect, kept

    def __len__(self):
        return len(self.params)

    def __iter__(self):
        return iter(zip(self.params, self.clouds, self.info))


@_lib.traced("proposals")
def proposals(lidar, mask=None, eps=0.5, min_points=10, max_points=None, max_clusters=512, n_angles=90, scale=2.0, latent=None, gates=None):
    """Rough boxes for align_many from a raw scan: `clusters`, `boxes`, then ONE HOST READ -- counts, offsets and rectangles in one copy, the
    only host synchronisation -- and on the host the gates and the poses (`starts_from_rect`).

    latent: REQUIRED, the start latent [L] of every proposal or one per accepted cluster [A][L] (the gates decide A, so a per-proposal
    array must match what comes out; a mismatch raises).  scale: the lattice scale of every start (the cube [-1, 1]^3 times scale, metres).
    gates: {'length': (min, max), 'width': (min, max), 'height': (min, max)} in metres on the rectangle's longer side, shorter side and y
    extent; a cluster outside any of them is dropped.  The rest: `clusters` and `boxes`.
    Returns a Proposals.  See the module docstring for what the defaults are."""
    if latent is None:
        raise ValueError("proposals: a start latent is required ([L], or one per proposal)")
    if not (float(scale) > 0 and math.isfinite(float(scale))):
        raise ValueError("proposals: the scale must be positive and finite")
    g = _gate(gates)
    cl = clusters(lidar, mask, eps, min_points, max_points, max_clusters)
    bx = boxes(None, cl, n_angles)
    dev, C = cl.label.device, cl.max_clusters
    host = torch.cat([cl.counts, cl.offsets, bx.rect.reshape(-1).view(torch.int32)]).cpu().numpy()          # the one host read
    counts, off = host[:4].copy(), host[4:5 + C].copy()
    kept = min(int(counts[2]), C)
    rect = host[5 + C:].view(np.float64).reshape(C, 8)[:kept].copy()
    total = int(off[kept])
    pts32 = cl.points if cl.points.dtype == torch.float32 else cl.points.float()
    gathered = pts32.index_select(0, cl.members[:total].long())
    yaw, trans, dims = starts_from_rect(rect, bx.dirs_host, scale)
    ok = np.nonzero(((dims >= g[None, :, 0]) & (dims <= g[None, :, 1])).all(1))[0] if kept else np.zeros(0, np.int64)
    A = len(ok)
    lat = latent.detach() if torch.is_tensor(latent) else torch.from_numpy(np.array(latent))
    lat = lat.to(torch.float32)
    if lat.dim() == 2 and int(lat.shape[0]) != A:
        raise ValueError("proposals: %d latents for %d accepted clusters" % (int(lat.shape[0]), A))
    if lat.dim() not in (1, 2):
        raise ValueError("proposals: the latent must be [L] or [A][L]")
    start = np.zeros((2, A, 5), np.float32)
    start[0, :, 0], start[1, :, 0] = yaw[ok], yaw[ok] + np.pi
    start[:, :, 1:4], start[:, :, 4] = trans[ok][None], float(scale)
    st = torch.from_numpy(start)
    if lat.is_cuda:
        st = _upload(st, dev)
    params = [[{"yaw": st[h, a, 0:1], "trans": st[h, a, 1:4], "scale": st[h, a, 4:5], "latent": lat if lat.dim() == 1 else lat[a]} for a in range(A)]
              for h in range(2)]
    clouds = [gathered[int(off[c]):int(off[c + 1])] for c in ok]
    centre = trans * float(scale)
    info = [{"cluster": int(c), "rect": rect[c].copy(), "n": int(off[c + 1] - off[c]), "dims": dims[c].copy(), "yaw": float(yaw[c]),
             "centre": centre[c].copy()} for c in ok]
    return Proposals(params[0], params[1], clouds, info, gathered, cl, bx, counts, off, rect, kept)
