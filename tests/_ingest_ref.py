"""Float64 / numpy restatements of the three frame-ingest kernels (csrc/ingest.hip), for the tests.

  frustum_planes, depth_map   utils/refinement.py:480-494 and :87-105 with cv2.undistortPoints / cv2.projectPoints as the plain pinhole
  match_boxes                 refine_css.py:101-114 around get_iou (utils/refinement.py:128-165)
  pil_bilinear_u8, css_input  utils/refinement.py:60-84: Pillow's 8-bit bilinear resample in integer arithmetic, ToTensor, Normalize

Nothing here imports the product: the CPU tests pin these functions to golden G19 and to PIL itself, the GPU tests pin the kernels to them.
"""
import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)
PRECISION_BITS = 22


def frustum_planes(K, l, t, r, b):
    """build_view_frustum: float32 [4][3] (top, right, bottom, left)"""
    K = np.asarray(K)
    corners = np.asarray([(l, t), (r - 1, t), (r - 1, b - 1), (l, b - 1)], dtype=np.float32)
    fx, fy, cx, cy = (np.float64(K[0, 0]), np.float64(K[1, 1]), np.float64(K[0, 2]), np.float64(K[1, 2]))
    rays = np.stack([(corners[:, 0] - cx) / fx, (corners[:, 1] - cy) / fy, np.ones(4)], 1).astype(np.float32)
    rays /= np.linalg.norm(rays, axis=1)[:, None]
    return np.stack((np.cross(rays[0], rays[1]), np.cross(rays[1], rays[2]), np.cross(rays[2], rays[3]), np.cross(rays[3], rays[0])))


def depth_map(lidar, K, w, h):
    """(depth float32 [h][w], winner int32 [h][w], kept, dropped): the last kept point in input order sets a pixel"""
    lidar = np.asarray(lidar)
    K = np.asarray(K, np.float64)
    pl = frustum_planes(K, 0, 0, w, h).astype(np.float64)
    p = lidar.astype(np.float64)
    dots = (pl[:, 0:1] * p[None, :, 0] + pl[:, 1:2] * p[None, :, 1]) + pl[:, 2:3] * p[None, :, 2]
    inside = np.logical_and.reduce(dots > 0, axis=0)
    idx = np.nonzero(inside)[0]
    q = p[idx]
    with np.errstate(all="ignore"):
        x = (K[0, 0] * (q[:, 0] / q[:, 2]) + K[0, 2]).astype(np.float32)
        y = (K[1, 1] * (q[:, 1] / q[:, 2]) + K[1, 2]).astype(np.float32)
    ok = (x > -1) & (x < w) & (y > -1) & (y < h)
    xi, yi = x[ok].astype(np.int32), y[ok].astype(np.int32)
    winner = np.full((h, w), -1, np.int32)
    np.maximum.at(winner, (yi, xi), idx[ok].astype(np.int32))
    depth = np.where(winner >= 0, lidar[np.maximum(winner, 0), 2].astype(np.float32), np.float32(0)).astype(np.float32)
    return depth, winner, int(ok.sum()), int((~ok).sum())


def get_iou(a, b, epsilon=1e-5):
    w = min(a[2], b[2]) - max(a[0], b[0])
    h = min(a[3], b[3]) - max(a[1], b[1])
    if (w < 0) or (h < 0):
        return 0.0
    inter = w * h
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter + epsilon)


def match_boxes(anno, det):
    """(best int32 [A], iou float64 [A], keep bool [A])"""
    anno, det = np.asarray(anno, np.float64).reshape(-1, 4), np.asarray(det, np.float64).reshape(-1, 4)
    best, iou = np.zeros(len(anno), np.int32), np.zeros(len(anno), np.float64)
    for i, a in enumerate(anno):
        v = [get_iou(d, a) for d in det]
        best[i] = int(np.argmax(v))
        iou[i] = v[best[i]]
    return best, iou, iou >= 0.5


def _coeffs(inS, outS):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the triangle filter: per output index (xmin, integer taps)"""
    scale = float(inS) / float(outS)
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    out = []
    for xx in range(outS):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        xmax = min(int(c + support + 0.5), inS)
        k = []
        ww = 0.0
        for x in range(xmax - xmin):
            wgt = max(0.0, 1.0 - abs((x + xmin - c + 0.5) * ss))
            k.append(wgt)
            ww += wgt
        kk = np.array([int(0.5 + (v / ww if ww != 0.0 else v) * (1 << PRECISION_BITS)) for v in k], np.int64)
        out.append((xmin, kk))
    return out


def _pass(img, outS):
    """one resample pass along axis 1 of a uint8 [rows][inS][C] array"""
    res = np.empty((img.shape[0], outS, img.shape[2]), np.uint8)
    src = img.astype(np.int64)
    for xx, (xmin, kk) in enumerate(_coeffs(img.shape[1], outS)):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, xmin:xmin + len(kk)], kk, axes=([1], [0]))
        res[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return res


def pil_bilinear_u8(img, size=128):
    """PIL.Image.fromarray(img).resize((size, size), Image.BILINEAR) of a uint8 [H][W][3] array, byte for byte: the horizontal pass over all
    rows, then the vertical pass over its uint8 result"""
    hp = _pass(np.ascontiguousarray(img), size)
    return _pass(hp.transpose(1, 0, 2), size).transpose(1, 0, 2)


def crop_u8(crop_bgr, mask=None):
    """(crop (* mask) * 255).astype(uint8) in float32, BGR -> RGB"""
    c = np.asarray(crop_bgr, np.float32)
    if mask is not None:
        c = c * np.asarray(mask, np.float32)[:, :, None]
    return np.ascontiguousarray((c * np.float32(255.0)).astype(np.uint8)[:, :, ::-1])


def css_input(crop_bgr, mask=None):
    """(im float32 [3][128][128], im_orig float32 [3][128][128], u8 [128][128][3]) of one crop"""
    u8 = pil_bilinear_u8(crop_u8(crop_bgr, mask))
    orig = (u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    im = ((orig - MEAN[:, None, None]) / STD[:, None, None]).astype(np.float32)
    return im, orig, u8
