"""Training crops for the CSS network from rasterised autolabels, on the device (csrc/crops.hip; DESIGN.md "Training crops").

    from sdflabel_amd.export import crops_many, Crop, CropWriter

crops_many   camera-frame meshes -> per annotation the NOCS image (uint8, coloured as the reference colours NOCS) and the RGB bytes of its
             label box, with the frame's annotations occluding each other; no host synchronisation
CropWriter   the reference's crops folder (crops.json, %05d_rgb.png, %05d_uvw.png) that datasets.crops.Crops reads; creates it or appends

The rasteriser of the verification decides which triangle wins a pixel (verify.raster_many); here the lattice-frame positions of that
triangle's vertices -- the decoder's canonical cube is the NOCS frame -- are interpolated perspective-correctly at the pixel.
"""
import json
import os

import numpy as np
import torch

from . import _lib
from .mesh import _host
from .pose import _upload
from . import verify as _verify
from .verify import FLAG_BEHIND, FLAG_INVALID, _intrinsics, label_windows  # noqa: F401  (the flag bits of Crop.flags)


class Crop:
    """One annotation's training crop.  `.uvw` uint8 [h][w][3] (NOCS bytes, zero where the annotation is not visible) and `.rgb` uint8
    [h][w][3] (or None) are device tensors of the box's shape; `.box` and `.window` are (l, t, r, b), half-open; `.counts` is an int32 [4]
    device tensor (box pixels, covered, visible, flag word) and `.flags` a 0-dim int32 device tensor: the rasteriser's flag word or-ed with
    the export's (bit 0: a triangle behind z_min was skipped; bit 1: an index or a window that does not fit -- the crop is then all zeros).
    `.latent`, `.intrinsics` (the frame's K) and `.extrinsics` (the label's cam_T) are None unless a pipeline filled them in
    (pipelines.frame.refine_frame does, for pipelines.export_crops.export_frame)."""

    def __init__(self, uvw, rgb, box, window, counts, flags, latent=None, intrinsics=None, extrinsics=None):
        self.uvw, self.rgb, self.box, self.window, self.counts, self.flags = uvw, rgb, box, window, counts, flags
        self.latent, self.intrinsics, self.extrinsics = latent, intrinsics, extrinsics


def _color_crop(c, lbox, cbox, b, dev):
    """the float32 BGR colours of the clipped box `cbox` as [n][3] on the device, from a crop of the label box's shape or the clipped box's"""
    t = c.detach() if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c))
    h, w = int(cbox[3] - cbox[1]), int(cbox[2] - cbox[0])
    lh, lw = int(lbox[3] - lbox[1]), int(lbox[2] - lbox[0])
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError("crops_many: colour crop %d has shape %s, not (h, w, 3)" % (b, tuple(t.shape)))
    if tuple(t.shape[:2]) == (lh, lw):
        t = t[cbox[1] - lbox[1]:cbox[3] - lbox[1], cbox[0] - lbox[0]:cbox[2] - lbox[0]]
    elif tuple(t.shape[:2]) != (h, w):
        raise ValueError("crops_many: colour crop %d has shape %s, neither its box's %s nor its clipped box's %s"
                         % (b, tuple(t.shape[:2]), (lh, lw), (h, w)))
    if dev is None:
        return None
    t = t.to(torch.float32).reshape(-1, 3)
    return t if t.is_cuda else _upload(t, dev)


@_lib.traced("crops_many")
def crops_many(meshes, K, boxes, image_size, colors=None, margin=0.25, occlusion=True, z_min=0.1, attributes=None, raster=None):
    """Training crops of all annotations of a frame.

    meshes: the refined shapes as camera-frame Mesh objects (Mesh.to_camera(), which hands the lattice-frame vertices on as
    `.lattice_vertices`).  K, image_size: the camera's intrinsics (host) and (W, H).  boxes: the 2-D labels [l, t, r, b]; each is taken
    outward to a half-open integer box and the mesh is rendered into verify.label_windows' window -- that box grown by `margin` and clipped
    to the image, the window verify_many renders into.  The crop is the label box clipped to the image.  colors: per annotation its float32
    BGR colour crop (h, w, 3) with values 0 ... 1, of the label box's shape or the clipped box's, on the device or the host; None: no
    `.rgb`.  attributes: per mesh a float32 [V][3] array to interpolate instead of `.lattice_vertices`.  raster: the verify.RasterBatch of these
    meshes in these windows (verify_many's `raster`), to be read instead of rendering again; one made with anything else is refused.

    NOCS bytes (DESIGN.md "Training crops"): at the rasteriser's winning triangle the three vertex attributes are interpolated
    perspective-correctly in float64 and coloured as the reference colours NOCS, byte = rint((x + 1) / 2 * 255); a labelled pixel is never
    (0, 0, 0), so the loader's mask u + v + w > 0 is exactly the set of labelled pixels.  occlusion: a pixel is labelled only where the
    annotation is the nearest of the frame's annotations (on an exact tie the lowest index).  AN OCCLUDER IS SEEN ONLY INSIDE ITS OWN
    WINDOW, and nothing but the annotations given occludes: poles, pedestrians and unlabelled cars do not.  With occlusion=False every
    covered pixel is labelled and an annotation's bytes do not depend on the batch.
    boxes equal to windows with margin=0 give a whole-window NOCS render.

    Returns a list of Crop.  The same bits on every run; no host synchronisation."""
    meshes = list(meshes)
    B = len(meshes)
    W, H = int(image_size[0]), int(image_size[1])
    if len(boxes) != B:
        raise ValueError("crops_many: %d meshes, %d boxes" % (B, len(boxes)))
    if colors is not None and len(colors) != B:
        raise ValueError("crops_many: %d colour crops for %d annotations" % (len(colors), B))
    if attributes is not None and len(attributes) != B:
        raise ValueError("crops_many: %d attribute arrays for %d meshes" % (len(attributes), B))
    if not float(margin) >= 0.0:
        raise ValueError("crops_many: the margin must not be negative (the crop's box lies inside the window rendered into)")
    if B == 0:
        return []
    att = []
    for b, m in enumerate(meshes):
        a = getattr(m, "lattice_vertices", None) if attributes is None else attributes[b]
        if a is None:
            raise ValueError("crops_many: mesh %d has no lattice_vertices (Mesh.to_camera() sets them) and no attributes were given" % b)
        if int(np.prod(tuple(a.shape))) != int(np.prod(tuple(m.vertices.shape))):
            raise ValueError("crops_many: mesh %d has %s vertices and attributes of shape %s" % (b, tuple(m.vertices.shape), tuple(a.shape)))
        att.append(a)
    lbox, win = label_windows(boxes, image_size, margin)
    box = np.stack([np.clip(lbox[:, 0], 0, W), np.clip(lbox[:, 1], 0, H), np.clip(lbox[:, 2], 0, W), np.clip(lbox[:, 3], 0, H)], 1)
    box[:, 2] = np.maximum(box[:, 2], box[:, 0])
    box[:, 3] = np.maximum(box[:, 3], box[:, 1])
    if colors is not None:
        for b, c in enumerate(colors):                       # (shapes only: refused before anything is launched)
            _color_crop(c, lbox[b], box[b], b, None)
    rb = _verify.raster_batch(meshes, K, win, image_size, z_min) if raster is None else raster.require("crops_many", meshes, K, win, image_size, z_min)
    dev = rb.device
    qoff = np.concatenate([[0], np.cumsum((box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1]))]).astype(np.int64)
    Q, P = int(qoff[-1]), rb.P
    table = _upload(torch.from_numpy(np.concatenate([qoff, box.astype(np.int32).reshape(-1).view(np.int64)])), dev)
    d_qoff, d_box = table[:B + 1], table[B + 1:].view(torch.int32)
    att = [(a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(torch.float32).reshape(-1, 3) for a in att]
    attr = torch.cat([a if a.is_cuda else _upload(a, dev) for a in att]).contiguous()
    packed = None
    if colors is not None:
        packed = torch.cat([_color_crop(c, lbox[b], box[b], b, dev) for b, c in enumerate(colors)]).contiguous()
    uvw = torch.empty((Q, 3), dtype=torch.uint8, device=dev)
    rgb = None if packed is None else torch.empty((Q, 3), dtype=torch.uint8, device=dev)
    owner = torch.empty((P,), dtype=torch.int32, device=dev) if occlusion else None
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    L, Pt, ck = _lib.lib(), _lib.ptr, _lib.check
    V, T = int(rb.vertices.shape[0]), int(rb.faces.shape[0])
    with _lib.guard(dev):
        st = _lib.stream_ptr()
        if occlusion:
            ck(L.sdfr_crop_owner(Pt(rb.mask) if P else None, Pt(rb.depth) if P else None, Pt(rb.d_win), Pt(rb.d_poff), P, B, W, H,
                                 Pt(owner) if P else None, st), "sdfr_crop_owner")
        ck(L.sdfr_crop_export(Pt(rb.vertices) if V else None, V, Pt(rb.faces) if T else None, T, Pt(attr) if V else None, Pt(rb.d_voff),
                              Pt(rb.d_toff), Pt(rb.d_win), Pt(rb.d_poff), P, Pt(rb.triangle) if P else None,
                              Pt(owner) if (occlusion and P) else None, Pt(d_box), Pt(d_qoff), Q, Pt(packed) if (packed is not None and Q) else None,
                              B, W, H, rb.k4, float(z_min), Pt(uvw) if Q else None, Pt(rgb) if (rgb is not None and Q) else None, Pt(flags), st),
           "sdfr_crop_export")
        ck(L.sdfr_crop_counts(Pt(rb.mask) if P else None, Pt(owner) if (occlusion and P) else None, Pt(rb.d_win), Pt(rb.d_poff), P,
                              Pt(d_box), Pt(d_qoff), Q, Pt(flags), B, W, H, Pt(counts), st), "sdfr_crop_counts")
    word = counts[:, 3] | rb.flags
    out = []
    for b in range(B):
        l, t, r, bt = (int(x) for x in box[b])
        q0, q1 = int(qoff[b]), int(qoff[b + 1])
        shape = (bt - t, r - l, 3)
        out.append(Crop(uvw[q0:q1].view(shape), None if rgb is None else rgb[q0:q1].view(shape), (l, t, r, bt), tuple(int(x) for x in win[b]),
                        counts[b], word[b]))
    return out


def crop_intrinsics(K, box):
    """the frame's 3x3 intrinsics with the principal point moved by the box's (l, t): the intrinsics of the crop"""
    fx, fy, cx, cy = _intrinsics(K)
    return np.array([[fx, 0.0, cx - float(box[0])], [0.0, fy, cy - float(box[1])], [0.0, 0.0, 1.0]], dtype=np.float64)


def _bytes_image(a, what):
    a = _host(a) if torch.is_tensor(a) else np.asarray(a)
    a = np.ascontiguousarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("CropWriter: %s must be a non-empty uint8 (h, w, 3) image, got %s %s" % (what, a.dtype, a.shape))
    return a


class CropWriter:
    """The reference's crops folder: crops.json = {str(idx): [{'latent', 'intrinsics', 'extrinsics', ...}]} beside %05d_rgb.png and
    %05d_uvw.png, as datasets.crops.Crops reads it.  A new folder is created; an existing one is appended to and the index continues.
    crops.json is written by close() (or on leaving the `with` block without an exception), through a temporary file and os.replace: a
    run that dies before close() leaves the old crops.json intact (and image files no entry points to).  Pillow is imported lazily and used
    for encoding only."""

    def __init__(self, path):
        self.path = str(path)
        os.makedirs(self.path, exist_ok=True)
        self._json = os.path.join(self.path, 'crops.json')
        self.gt = {}
        if os.path.isfile(self._json):
            with open(self._json, 'r') as f:
                self.gt = json.load(f)
        self.next = max([int(k) for k in self.gt] + [-1]) + 1
        self.closed = False

    def __len__(self):
        return len(self.gt)

    def add(self, crop, latent, intrinsics, extrinsics, **meta):
        """One download of `crop` (a Crop, or any object with `.uvw`, `.rgb` and `.box` as device tensors or host arrays) and two PNG files.
        latent: the raw refined latent the mesh was decoded from.  intrinsics: the FRAME's K (3x3 or fx, fy, cx, cy); the entry holds it with
        the principal point moved by the box's (l, t).  extrinsics: the label's 4x4 cam_T.  meta: further JSON-serialisable fields of the
        entry.  Returns the index written."""
        from PIL import Image                                  # encoding only
        if self.closed:
            raise ValueError("CropWriter: the writer is closed")
        if crop.rgb is None:
            raise ValueError("CropWriter: the crop has no rgb image (crops_many(colors=...))")
        if torch.is_tensor(crop.uvw) and torch.is_tensor(crop.rgb) and crop.uvw.is_cuda and crop.rgb.is_cuda:
            both = torch.stack([crop.uvw, crop.rgb]).cpu().numpy()                          # the one download
            uvw, rgb = both[0], both[1]
        else:
            uvw, rgb = crop.uvw, crop.rgb
        uvw, rgb = _bytes_image(uvw, "uvw"), _bytes_image(rgb, "rgb")
        if uvw.shape != rgb.shape:
            raise ValueError("CropWriter: an RGB image of %s and a UVW image of %s" % (rgb.shape, uvw.shape))
        lat = np.asarray(_host(latent), dtype=np.float64).reshape(-1)
        ext = np.asarray(_host(extrinsics), dtype=np.float64).reshape(4, 4)
        entry = {'latent': lat.tolist(), 'intrinsics': crop_intrinsics(intrinsics, crop.box).tolist(), 'extrinsics': ext.tolist()}
        entry.update(meta)
        json.dumps(entry)                                      # refuse what cannot be written before any file exists
        idx = self.next
        Image.fromarray(rgb, 'RGB').save(os.path.join(self.path, '{:05d}_rgb.png'.format(idx)))
        Image.fromarray(uvw, 'RGB').save(os.path.join(self.path, '{:05d}_uvw.png'.format(idx)))
        self.gt[str(idx)] = [entry]
        self.next = idx + 1
        return idx

    def close(self):
        if self.closed:
            return
        tmp = self._json + '.tmp'
        with open(tmp, 'w') as f:
            json.dump(self.gt, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, self._json)
        self.closed = True

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        return False
