"""Verification of refined autolabels on the device (csrc/verify.hip; DESIGN.md "Verification").

    from sdflabel_amd.verify import raster_many, raster_batch, band_counts, verify_many

raster_many   camera-frame meshes -> mask, depth and winning triangle in each mesh's own window of the image, by an exact rasteriser whose
              result is defined independently of the schedule
raster_batch  the same launches with the result kept packed (RasterBatch): what verify_many and export.crops_many read, and take as
              `raster=` so that a frame is rendered once
band_counts   lidar points taken to each annotation's lattice frame, the decoder there, and the integer counts of points in a band round
              the surface
verify_many   both, the counts of the rendered mask against the 2-D label, ONE host read, and a verdict per annotation

An autolabel is accepted when the rendered shape overlaps its 2-D label (projective test) and most of the lidar points in the label's
frustum lie in a narrow band round the refined surface (geometric test).  Nothing here filters: the caller decides what to drop.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .mesh import STAGING_BYTES, _decoder_mode, _host
from .pose import _upload

FLAG_BEHIND, FLAG_INVALID = 1, 2          # bits of a raster's flag word: a triangle behind z_min was skipped; a bad face index / window


class Raster:
    """One mesh rendered into its window.  `.mask` uint8 (0 / 1), `.depth` float32 (0 where uncovered) and `.triangle` int32 (index local to
    the mesh, -1 where uncovered) are device tensors of the window's shape (b - t, r - l); `.window` is (l, t, r, b), half-open; `.flags` is a
    0-dim int32 device tensor (bit 0: a triangle with a vertex at Z <= z_min was skipped; bit 1: a face index outside the mesh)."""

    def __init__(self, mask, depth, triangle, window, flags):
        self.mask, self.depth, self.triangle, self.window, self.flags = mask, depth, triangle, window, flags


def _intrinsics(K):
    """(fx, fy, cx, cy) as Python floats (doubles) of a 3x3 matrix or a 4-sequence on the host"""
    k = np.asarray(_host(K), dtype=np.float64)
    if k.shape == (4,):
        return tuple(float(x) for x in k)
    if k.shape[-2:] != (3, 3):
        raise ValueError("verify: K must be 3x3 intrinsics or (fx, fy, cx, cy)")
    k = k.reshape(3, 3)
    return float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])


class RasterBatch:
    """A frame's meshes rendered into their windows, packed: what raster_batch made and what every stage that reads the rasters takes.
    `.mask` uint8 [P], `.depth` float32 [P], `.triangle` int32 [P] and `.flags` int32 [B] are the rasteriser's packed outputs, `.vertices`
    float32 [V][3] and `.faces` int32 [T][3] its packed inputs, `.d_voff`, `.d_toff`, `.d_poff` (int64 [B + 1]) and `.d_win` (int32 [4 B]) the
    device tables; `.windows` int64 [B][4] and `.poff` int64 [B + 1] are their host copies.  `.P`, `.W`, `.H`, `.device` as passed to the
    kernels.  `.k4` (four doubles), `.z_min` and `.sizes` (per mesh its vertex and face count) say what the batch was made with."""

    def __init__(self, mask, depth, triangle, flags, vertices, faces, d_voff, d_toff, d_poff, d_win, windows, poff, P, W, H, device, k4, z_min, sizes):
        self.mask, self.depth, self.triangle, self.flags, self.vertices, self.faces = mask, depth, triangle, flags, vertices, faces
        self.d_voff, self.d_toff, self.d_poff, self.d_win, self.windows, self.poff = d_voff, d_toff, d_poff, d_win, windows, poff
        self.P, self.W, self.H, self.device, self.k4, self.z_min, self.sizes = P, W, H, device, k4, z_min, sizes

    def rasters(self):
        """one Raster per mesh: views of the packed outputs"""
        out = []
        for b, (l, t, r, bt) in enumerate(self.windows.tolist()):
            p0, p1 = int(self.poff[b]), int(self.poff[b + 1])
            shape = (bt - t, r - l)
            out.append(Raster(self.mask[p0:p1].view(shape), self.depth[p0:p1].view(shape), self.triangle[p0:p1].view(shape), (l, t, r, bt),
                              self.flags[b]))
        return out

    def mask_counts(self, label=None):
        """int32 [B][8] on the device: area, tight box l t r b, label area, intersection, flag"""
        B = int(self.windows.shape[0])
        out = torch.empty((B, 8), dtype=torch.int32, device=self.device)
        if B:
            with _lib.guard(self.device):
                _lib.check(_lib.lib().sdfr_verify_mask_counts(_lib.ptr(self.mask) if self.P else None, _lib.ptr(label), _lib.ptr(self.d_win),
                                                              _lib.ptr(self.d_poff), self.P, B, self.W, self.H, _lib.ptr(out), _lib.stream_ptr()),
                           "sdfr_verify_mask_counts")
        return out

    def require(self, who, meshes, K, windows, image_size, z_min):
        """refuse, on the host and before any launch, a batch that is not the one raster_batch(meshes, K, windows, image_size, z_min) makes"""
        sizes = [(int(m.vertices.shape[0]), int(m.faces.shape[0])) for m in meshes]
        made = (("meshes", self.sizes, sizes), ("image size", (self.W, self.H), (int(image_size[0]), int(image_size[1]))),
                ("intrinsics", tuple(self.k4), _intrinsics(K)), ("z_min", self.z_min, float(z_min)),
                ("windows", self.windows.tolist(), np.asarray(windows, dtype=np.int64).reshape(-1, 4).tolist()))
        for what, has, wants in made:
            if has != wants:
                raise ValueError("%s: the raster batch was made for other %s (%s, not %s)" % (who, what, has, wants))
        return self


def raster_batch(meshes, K, windows, image_size, z_min=0.1):
    """The launches of raster_many, kept packed: a RasterBatch, which verify_many and export.crops_many also take as `raster=` so that a
    frame is rendered once.  Arguments as raster_many's."""
    L = _lib.lib()
    meshes = list(meshes)
    W, H = int(image_size[0]), int(image_size[1])
    B = len(meshes)
    win = np.asarray(windows, dtype=np.int64).reshape(-1, 4)
    if win.shape[0] != B:
        raise ValueError("verify: %d meshes, %d windows" % (B, win.shape[0]))
    for m in meshes:
        if getattr(m, "frame", None) != "camera":
            raise ValueError("verify: the rasteriser takes camera-frame meshes (Mesh.to_camera()); got a %r-frame mesh" % getattr(m, "frame", None))
        if not m.vertices.is_cuda:
            raise _lib.SdfrError("raster_many runs on the GPU only; there is no CPU fallback")
    if B and not ((0 <= win[:, 0]) & (win[:, 0] <= win[:, 2]) & (win[:, 2] <= W) & (0 <= win[:, 1]) & (win[:, 1] <= win[:, 3]) & (win[:, 3] <= H)).all():
        raise ValueError("verify: every window [l, t, r, b) must be clipped to the %d x %d image" % (W, H))
    k4 = (ctypes.c_double * 4)(*_intrinsics(K))
    dev = meshes[0].vertices.device if B else torch.device("cuda", torch.cuda.current_device())
    sizes = [(int(m.vertices.shape[0]), int(m.faces.shape[0])) for m in meshes]
    voff = np.concatenate([[0], np.cumsum([v for v, _ in sizes])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([t for _, t in sizes])]).astype(np.int64)
    poff = np.concatenate([[0], np.cumsum((win[:, 2] - win[:, 0]) * (win[:, 3] - win[:, 1]))]).astype(np.int64)
    V, T, P = int(voff[-1]), int(toff[-1]), int(poff[-1])
    table = _upload(torch.from_numpy(np.concatenate([voff, toff, poff, win.astype(np.int32).reshape(-1).view(np.int64) if B else
                                                     np.zeros(0, np.int64)])), dev)
    n1 = B + 1
    d_voff, d_toff, d_poff = table[:n1], table[n1:2 * n1], table[2 * n1:3 * n1]
    d_win = table[3 * n1:].view(torch.int32)
    verts = torch.cat([m.vertices.detach().float().reshape(-1, 3) for m in meshes]).contiguous() if B else torch.zeros((0, 3), device=dev)
    faces = torch.cat([m.faces.detach().to(torch.int32).reshape(-1, 3) for m in meshes]).contiguous() if B else \
        torch.zeros((0, 3), dtype=torch.int32, device=dev)
    keys = torch.empty((P,), dtype=torch.int64, device=dev)                         # the rasteriser's workspace
    mask = torch.empty((P,), dtype=torch.uint8, device=dev)
    depth = torch.empty((P,), dtype=torch.float32, device=dev)
    tri = torch.empty((P,), dtype=torch.int32, device=dev)
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    Pt = _lib.ptr
    if B:
        with _lib.guard(dev):
            _lib.check(L.sdfr_mesh_raster(Pt(verts) if V else None, V, Pt(faces) if T else None, T, Pt(d_voff), Pt(d_toff), Pt(d_win), Pt(d_poff), P,
                                          B, W, H, k4, float(z_min), Pt(keys) if P else None, Pt(mask) if P else None, Pt(depth) if P else None,
                                          Pt(tri) if P else None, Pt(flags), _lib.stream_ptr()), "sdfr_mesh_raster")
    return RasterBatch(mask, depth, tri, flags, verts, faces, d_voff, d_toff, d_poff, d_win, win, poff, P, W, H, dev, k4, float(z_min), sizes)


@_lib.traced("raster_many")
def raster_many(meshes, K, windows, image_size, z_min=0.1):
    """Render camera-frame meshes into windows of one image.

    meshes: sdflabel_amd.mesh.Mesh objects in the CAMERA frame (Mesh.to_camera(); a lattice-frame mesh is refused).  K: the camera's 3x3
    intrinsics or (fx, fy, cx, cy), on the host.  windows: per mesh a half-open integer window [l, t, r, b) inside the image (an empty one
    is legal).  image_size: (W, H).  z_min: triangles with a vertex at Z <= z_min are skipped and flag bit 0 is set.

    The result is defined (DESIGN.md "Verification"): float64 pinhole projection of the float32 vertices, pixel (x, y) sampled at the point
    (x, y), inclusive edges, both windings, perspective-correct depth, the nearest depth wins and on an exact tie the lowest triangle
    index.  The same bits on every run and in every batch.  Returns a list of Raster; no host synchronisation."""
    return raster_batch(meshes, K, windows, image_size, z_min).rasters()


def _pose_rows(params_list, device):
    """(pose float32 [B][6] = cos(yaw), sin(yaw), trans, scale; latents float32 [B][L]) on the device.  The cosine and sine are float32
    functions of the float32 yaw, as frame.assemble_labels takes them: of host parameters on the host (the label's own bits), of device
    parameters on the device, without reading them."""
    keys = ("yaw", "trans", "scale", "latent")
    on_host = all(not (torch.is_tensor(p[k]) and p[k].is_cuda) for p in params_list for k in keys)

    def flat(p, k, n):
        t = torch.as_tensor(np.asarray(p[k])) if not torch.is_tensor(p[k]) else p[k].detach()
        return t.reshape(-1)[:n].to(torch.float32) if n else t.reshape(-1).to(torch.float32)

    where = "cpu" if on_host else device
    yaw = torch.stack([flat(p, "yaw", 1).to(where) for p in params_list]).reshape(-1)
    trans = torch.stack([flat(p, "trans", 3).to(where) for p in params_list])
    scale = torch.stack([flat(p, "scale", 1).to(where) for p in params_list]).reshape(-1, 1)
    lat = torch.stack([flat(p, "latent", 0).to(where) for p in params_list])
    pose = torch.cat([torch.cos(yaw)[:, None], torch.sin(yaw)[:, None], trans, scale], 1).contiguous()
    if on_host:
        return _upload(pose, device), _upload(lat.contiguous(), device)
    return pose, lat.contiguous()


def _band_packed(dsdf, params_list, clouds, band, staging_bytes, keep_rows=False):
    L = _lib.lib()
    dev = next(dsdf.parameters()).device
    if dev.type != "cuda":
        raise _lib.SdfrError("band_counts runs on the GPU only; there is no CPU fallback")
    B = len(params_list)
    if len(clouds) != B:
        raise ValueError("verify: %d parameter sets, %d clouds" % (B, len(clouds)))
    counts = torch.zeros((B, 3), dtype=torch.int32, device=dev)
    if B == 0:
        return dict(counts=counts)
    pts = []
    for c in clouds:
        t = c.detach() if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32))
        t = t.reshape(-1, 3).to(torch.float32)
        pts.append(t if t.is_cuda else _upload(t, dev))
    ptoff = np.concatenate([[0], np.cumsum([int(t.shape[0]) for t in pts])]).astype(np.int64)
    N = int(ptoff[-1])
    points = torch.cat(pts).contiguous()
    d_ptoff = _upload(torch.from_numpy(ptoff), dev)
    pose, lat = _pose_rows(params_list, dev)
    Ld = int(lat.shape[1])
    if Ld != int(dsdf.latent_size):
        raise ValueError("verify: latents of size %d for a decoder of latent size %d" % (Ld, dsdf.latent_size))
    handle, fwd, _ = _decoder_mode(dsdf, dev)
    NI = Ld + 3
    budget = max(128, int(staging_bytes) // (4 * NI) // 128 * 128)                 # rows in flight
    sdf = torch.empty((N,), dtype=torch.float32, device=dev)
    in_cube = torch.empty((N,), dtype=torch.uint8, device=dev)
    rows = torch.empty((N if keep_rows else min(N, budget), NI), dtype=torch.float32, device=dev)
    Pt, ck = _lib.ptr, _lib.check
    with _lib.guard(dev):
        st = _lib.stream_ptr()
        for r0 in range(0, N, budget):
            n = min(budget, N - r0)
            chunk = rows[r0:r0 + n] if keep_rows else rows
            ck(L.sdfr_verify_point_rows(Pt(points), N, Pt(d_ptoff), B, Pt(pose), Pt(lat), Ld, r0, n, Pt(chunk), Pt(in_cube), st),
               "sdfr_verify_point_rows")
            ck(fwd(handle.h, Pt(chunk), n, Pt(sdf[r0:]), None, st), fwd.__name__)
        ck(L.sdfr_verify_band_counts(Pt(sdf) if N else None, Pt(in_cube) if N else None, N, Pt(d_ptoff), B, Pt(pose), float(band), Pt(counts), st),
           "sdfr_verify_band_counts")
    return dict(counts=counts, sdf=sdf, in_cube=in_cube, rows=rows if keep_rows else None, pose=pose, latents=lat, ptoff=ptoff, points=points,
                d_ptoff=d_ptoff)


@_lib.traced("band_counts")
def band_counts(dsdf, params_list, clouds, band=0.2, staging_bytes=STAGING_BYTES, return_details=False):
    """The geometric test's counts.

    params_list: per annotation the refined {'yaw', 'trans', 'scale', 'latent'} as Optimizer.optimize_many leaves them; THE LATENT GOES TO
    THE DECODER RAW, as in labels_many and meshes_many.  clouds: per annotation the camera-frame lidar points [n][3] of its frustum.
    Every point p is taken to the annotation's lattice frame, x = diag(1, -1, 1) rot_yaw^T (p / scale - trans) in float64 rounded once --
    the inverse of Mesh.to_camera --, the decoder (the forward its mlp_precision picks) is evaluated at latent || x in chunks of at most
    staging_bytes of input rows, and a point counts as in the band when x lies in [-1, 1]^3 and |sdf| * scale < band (float32; band in the
    units of the cloud, metres for KITTI).  Points outside the cube are out of the band whatever the decoder says there.
    Returns int32 [B][3] on the device: n_pts, n_cube, n_band.  No host synchronisation.  With return_details also a dict of the rows, the
    decoder's values, the in-cube bytes, the pose rows and the point offsets."""
    d = _band_packed(dsdf, list(params_list), list(clouds), band, staging_bytes, keep_rows=return_details)
    return (d["counts"], d) if return_details else d["counts"]


def label_windows(boxes, image_size, margin=0.25):
    """(label boxes, windows) as int64 [B][4]: a label box [l, t, r, b] is taken outward to integers (half-open), and its window is the box
    grown by ceil(margin * width) / ceil(margin * height) on every side, clipped to the image (W, H)."""
    W, H = int(image_size[0]), int(image_size[1])
    bx = np.asarray([np.asarray(_host(b), dtype=np.float64).reshape(-1)[:4] for b in boxes], dtype=np.float64).reshape(-1, 4)
    box = np.stack([np.floor(bx[:, 0]), np.floor(bx[:, 1]), np.ceil(bx[:, 2]), np.ceil(bx[:, 3])], 1).astype(np.int64)
    mw = np.ceil(float(margin) * np.maximum(box[:, 2] - box[:, 0], 0)).astype(np.int64)
    mh = np.ceil(float(margin) * np.maximum(box[:, 3] - box[:, 1], 0)).astype(np.int64)
    win = np.stack([np.clip(box[:, 0] - mw, 0, W), np.clip(box[:, 1] - mh, 0, H), np.clip(box[:, 2] + mw, 0, W), np.clip(box[:, 3] + mh, 0, H)], 1)
    win[:, 2] = np.maximum(win[:, 2], win[:, 0])
    win[:, 3] = np.maximum(win[:, 3], win[:, 1])
    return box, win


def _box_iou(a, b):
    """IoU of two half-open integer boxes l, t, r, b in float64"""
    aw, ah, bw, bh = max(a[2] - a[0], 0), max(a[3] - a[1], 0), max(b[2] - b[0], 0), max(b[3] - b[1], 0)
    iw, ih = max(min(a[2], b[2]) - max(a[0], b[0]), 0), max(min(a[3], b[3]) - max(a[1], b[1]), 0)
    union = float(aw * ah + bw * bh - iw * ih)
    return float(iw * ih) / union if union > 0 else 0.0


def _pack_labels(label_masks, box, win, poff, dev):
    """the label masks as one uint8 [P] laid out like the rendered masks; a mask may have its window's shape or its label box's shape (then
    it is placed into the window, cut where the box leaves the image); None entries stay zero"""
    P = int(poff[-1])
    out = torch.zeros((P,), dtype=torch.uint8, device=dev)
    for b, m in enumerate(label_masks):
        if m is None:
            continue
        l, t, r, bt = (int(x) for x in win[b])
        h, w = bt - t, r - l
        m = (m.detach() if torch.is_tensor(m) else torch.from_numpy(np.ascontiguousarray(m)))
        m = (m != 0).to(torch.uint8)
        m = m if m.is_cuda else _upload(m, dev)
        view = out[int(poff[b]):int(poff[b + 1])].view(h, w)
        if tuple(m.shape) == (h, w):
            view.copy_(m)
            continue
        bl, btop, br, bb = (int(x) for x in box[b])
        if tuple(m.shape) != (bb - btop, br - bl):
            raise ValueError("verify: label mask %d has shape %s, neither its window's %s nor its box's %s"
                             % (b, tuple(m.shape), (h, w), (bb - btop, br - bl)))
        x0, y0, x1, y1 = max(bl, l), max(btop, t), min(br, r), min(bb, bt)
        if x1 > x0 and y1 > y0:
            view[y0 - t:y1 - t, x0 - l:x1 - l].copy_(m[y0 - btop:y1 - btop, x0 - bl:x1 - bl])
    return out


@_lib.traced("verify_many")
def verify_many(dsdf, params_list, meshes, clouds, K, boxes, image_size, label_masks=None, margin=0.25, band=0.2, min_iou=0.7, min_share=0.6,
                iou='box', z_min=0.1, staging_bytes=STAGING_BYTES, raster=None):
    """The two tests of an autolabel, for all annotations of a frame.

    params_list, clouds: band_counts'.  meshes: the refined shapes as camera-frame Mesh objects.  K, image_size: the camera's intrinsics
    (host) and (W, H).  boxes: the 2-D labels [l, t, r, b]; each is taken outward to a half-open integer box, and the mesh is rendered into
    that box grown by `margin` of its width / height on every side and clipped to the image (label_windows).  label_masks: per annotation
    a 2-D uint8 / bool label mask of the window's shape -- or of the label box's shape, which is placed into the window -- or None.
    raster: the RasterBatch of these meshes in these windows (raster_batch(meshes, K, label_windows(boxes, image_size, margin)[1],
    image_size, z_min)), to be read instead of rendering again; one made with anything else is refused with a ValueError.

    ONE host read, of all the counts.  Returns per annotation a dict:
      iou_box    IoU of the tight box of the rendered mask and the label box, both half-open integer boxes, float64 on the host
      iou_mask   pixel IoU of the rendered mask and the label mask (None without a label mask)
      area, mask_box   covered pixels and their tight half-open box [l, t, r, b] (zeros for none)
      n_pts, n_cube, n_band, share   band_counts' figures and n_band / n_pts (0.0 without points)
      flags      the rasteriser's flag word        window   the window rendered into
      ok, why    the verdict and the list of failed constraints among 'no_points', 'empty_mask', 'iou', 'share'
    The verdict is iou >= min_iou and share >= min_share, with iou = iou_box, or iou_mask for iou='mask'.

    min_iou = 0.7, min_share = 0.6 and band = 0.2 (metres) are the method's published operating point AS RECALLED: the paper was not at hand
    when this was written, so check them against it before relying on them.  They are parameters, nothing else depends on them."""
    if iou not in ('box', 'mask'):
        raise ValueError("verify_many: iou must be 'box' or 'mask'")
    params_list, meshes, clouds = list(params_list), list(meshes), list(clouds)
    B = len(meshes)
    if not (len(params_list) == len(clouds) == len(boxes) == B):
        raise ValueError("verify_many: %d meshes, %d parameter sets, %d clouds, %d boxes" % (B, len(params_list), len(clouds), len(boxes)))
    if label_masks is not None and len(label_masks) != B:
        raise ValueError("verify_many: %d label masks for %d annotations" % (len(label_masks), B))
    if iou == 'mask' and (label_masks is None or any(m is None for m in label_masks)):
        raise ValueError("verify_many: iou='mask' needs a label mask for every annotation")
    if B == 0:
        return []
    box, win = label_windows(boxes, image_size, margin)
    rb = raster_batch(meshes, K, win, image_size, z_min) if raster is None else raster.require("verify_many", meshes, K, win, image_size, z_min)
    label = None if label_masks is None else _pack_labels(label_masks, box, win, rb.poff, rb.device)
    c8 = rb.mask_counts(label)
    c3 = band_counts(dsdf, params_list, clouds, band=band, staging_bytes=staging_bytes)
    host = torch.cat([c8, c3.to(c8.device), rb.flags[:, None]], 1).cpu().numpy().astype(np.int64)          # the one host read
    out = []
    for b in range(B):
        area, mbox, la, inter, bad = int(host[b, 0]), [int(x) for x in host[b, 1:5]], int(host[b, 5]), int(host[b, 6]), int(host[b, 7])
        n_pts, n_cube, n_band, flags = int(host[b, 8]), int(host[b, 9]), int(host[b, 10]), int(host[b, 11]) | bad
        iou_box = _box_iou(mbox, [int(x) for x in box[b]]) if area else 0.0
        iou_mask = None
        if label_masks is not None and label_masks[b] is not None:
            union = area + la - inter
            iou_mask = float(inter) / float(union) if union > 0 else 0.0
        share = float(n_band) / float(n_pts) if n_pts > 0 else 0.0
        used = iou_box if iou == 'box' else iou_mask
        why = []
        if n_pts == 0:
            why.append('no_points')
        if area == 0:
            why.append('empty_mask')
        if not used >= float(min_iou):
            why.append('iou')
        if not share >= float(min_share):
            why.append('share')
        out.append({'iou_box': iou_box, 'iou_mask': iou_mask, 'area': area, 'mask_box': mbox, 'n_pts': n_pts, 'n_cube': n_cube, 'n_band': n_band,
                    'share': share, 'flags': flags, 'window': tuple(int(x) for x in win[b]), 'ok': not why, 'why': why})
    return out
