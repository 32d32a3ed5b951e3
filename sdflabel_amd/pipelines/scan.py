"""Labels from a lidar scan and a shape prior alone: scan -> remove_road -> proposals -> align_many -> labels_many.

The lidar-only branch (encode, complete, align) fitted pose and shape to a cloud from a rough box, but every caller took that box from the
CSS refinement, which needs 2-D annotations and a CSS network.  cluster.proposals makes the box from the scan itself; label_scan chains it
with the steps that were there.  The reference has no counterpart to this pipeline.

Nothing here claims anything about label quality on real scans: all defaults of the stages are parameters without a claimed operating
point (cluster.py, align.py).
"""
import numpy as np
import torch

from .. import frame as FR
from ..align import align_many
from ..cluster import proposals
from ..pose import _upload


def choose(loss, A):
    """bool [A] on the device: True where the second hypothesis (yaw + pi, rows A ... 2A - 1 of the batch) has the strictly lower loss; a tie
    takes the first, a NaN loss loses (two NaNs: the first)."""
    l0, l1 = loss[:A], loss[A:2 * A]
    return (l1 < l0) | (torch.isnan(l0) & ~torch.isnan(l1))


def pinhole_extents(props, K):
    """float32 [A][4] = min u, max u, min v, max v of every accepted cluster's own points through the pinhole K (sdfr_point_extents), on the
    device; no synchronisation"""
    A = len(props)
    dev = props.gathered.device
    off = np.array([int(props.offsets[i["cluster"]]) for i in props.info], np.int64)
    cnt = np.array([i["n"] for i in props.info], np.int32)
    Kh = np.tile(np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, np.float32).reshape(1, 9), (A, 1))
    ext, _ = FR.point_extents(props.gathered, _upload(torch.from_numpy(off), dev), _upload(torch.from_numpy(cnt), dev), int(cnt.max()), A,
                              K=_upload(torch.from_numpy(Kh), dev))
    return ext[:, 6:10]


def label_scan(dsdf, grid, lidar, K, w, h, world_to_cam, latent, remove_road=True, cluster_kw=None, align_kw=None, *, search=None):
    """KITTI labels of one scan from the lidar and the shape prior `dsdf` alone.

    lidar [N][3], camera frame; K, w, h: the camera (the frustum of remove_road, the labels' 2-D boxes); world_to_cam: the 4x4 p_WC of
    labels_many; latent: the start latent of every proposal ([L]); cluster_kw: keyword arguments of cluster.proposals (eps, min_points,
    max_points, max_clusters, n_angles, scale, gates); align_kw: those of align.align_many.  Steps:
      1. frame.remove_road -- or, with remove_road=False, every point (the frustum is not cut then: cut it before, or let the gates do it);
      2. cluster.proposals on the kept points;
      3. align_many on both yaw hypotheses of every proposal in ONE batch of 2 A shapes (rows 0 ... A - 1: yaw, rows A ... 2 A - 1: yaw + pi);
      4. per proposal the hypothesis of the lower Aligned.loss -- a tie takes the first, a NaN loss loses (`choose`, on the device);
      5. frame.labels_many, each label's 2-D box [l, t, r, b] being the pinhole extents of the cluster's own points, clipped to the image.
    HOST SYNCHRONISATIONS: 2 + ceil(A / 16) for A accepted proposals -- one in proposals (counts, offsets, rectangles), one here (the 2-D
    boxes and the choice, one copy), one per chunk of 16 annotations in labels_many; remove_road and align_many make none.  With A == 0 it is
    the one of proposals.
    search: None, or align_many's search dict (`codes`, `yaws`, `keep`, `rows`): steps 3 and 4 then are align_many(props.params, props.clouds,
    search=search) -- search.search_poses over codes x yaw offsets on every proposal's box, the fit of the kept starts, search.choose --;
    `latent` is not used as a start, stages['fits'] is that Aligned (with `.found`, `.chosen`, `.fits`), stages['second'] stays empty and
    stages['chosen'] holds the chosen ranks on the host.  The synchronisations are the same.
    Returns (labels, stages): labels in the dict shape frame.frame_dict makes; stages = {'keep', 'proposals' (with its clusters and
    rectangles), 'fits' (the Aligned of the 2 A-batch, or None), 'second' (the choice, bool [A] on the host), 'params' (the chosen
    parameters, device tensors), 'bboxes', 'labels' (labels_many's tuples)}."""
    keep = FR.remove_road(lidar, K, w, h) if remove_road else None
    props = proposals(lidar, keep, latent=latent, **(cluster_kw or {}))
    A = len(props)
    stages = {"keep": keep, "proposals": props, "fits": None, "second": np.zeros(0, bool), "params": [], "bboxes": [], "labels": []}
    if A == 0:
        return FR.frame_dict([]), stages
    if search is not None:
        fits = align_many(dsdf, props.params, props.clouds, search=search, **(align_kw or {}))
        theta, lat, second = fits.theta, fits.latents, fits.chosen
    else:
        fits = align_many(dsdf, props.params + props.flipped, props.clouds + props.clouds, **(align_kw or {}))
        second = choose(fits.loss, A)
        theta = torch.where(second[:, None], fits.theta[A:], fits.theta[:A])
        lat = torch.where(second[:, None], fits.latents[A:], fits.latents[:A])
    uv = pinhole_extents(props, K)
    host = torch.cat([uv.reshape(-1), second.float()]).cpu().numpy()                     # the one host read of this function
    uv, sec = host[:4 * A].reshape(A, 4), host[4 * A:] != 0
    if search is not None:
        stages["chosen"], sec = host[4 * A:].astype(np.int64), np.zeros(0, bool)
    bboxes = [np.array([np.clip(u0, 0, w), np.clip(v0, 0, h), np.clip(u1, 0, w), np.clip(v1, 0, h)], np.float32) for u0, u1, v0, v1 in uv]
    params = [{"yaw": theta[a, 0:1], "trans": theta[a, 1:4], "scale": theta[a, 4:5], "latent": lat[a]} for a in range(A)]
    labels = FR.labels_many(dsdf, grid, params, world_to_cam, bboxes)
    stages.update(fits=fits, second=sec, params=params, bboxes=bboxes, labels=labels)
    return FR.frame_dict(labels), stages
