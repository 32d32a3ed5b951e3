"""Labels from several lidar scans of the same scene and a shape prior alone: per scan remove_road -> proposals, one align_many batch over
every proposal of every scan, association of the proposals into tracks, align_tracks -- one latent and one scale per object over all its
views --, labels_many per scan.

pipelines.scan.label_scan sees every object from one sensor position.  A drive shows it from several; what the views share is the object,
and track.align_tracks fits that part once.  The reference has no counterpart to this pipeline.

Nothing here claims anything about label quality on real drives: the stages' defaults and `gate` are parameters without a claimed operating
point (cluster.py, align.py, track.py).  The association knows centre distances and nothing else -- no motion model, no appearance.
"""
import numpy as np
import torch

from .. import frame as FR
from ..align import align_many
from ..cluster import proposals
from ..pose import _upload
from ..track import align_tracks
from .scan import choose, pinhole_extents


def associate(centres, gate=2.0):
    """Proposals of consecutive scans into tracks, by centre distance alone.  Plain numpy, deterministic.

    centres: per scan the world-frame centres [n_i][3] of its proposals.  Scans are taken in order; a scan's proposals are matched greedily
    to the LAST centres of the tracks opened so far: the pairs within `gate` metres in ascending distance, ties by the lower track, then by
    the lower proposal; a track takes at most one proposal of a scan and a proposal one track; a proposal left over opens a track (in
    proposal order).  A track that finds no proposal in a scan stays open with the centre it has.  `gate` has no claimed operating point.
    Returns (tracks, assigned): tracks[t] the list of (scan, proposal) of track t in scan order, assigned[i] int64 [n_i] the track of every
    proposal of scan i."""
    gate = float(gate)
    if not gate >= 0:
        raise ValueError("associate: the gate must not be negative")
    tracks, last, assigned = [], [], []
    for i, c in enumerate(centres):
        c = np.asarray(c, np.float64).reshape(-1, 3)
        mine = np.full((len(c),), -1, np.int64)
        if len(c) and last:
            d = np.sqrt(((np.asarray(last)[:, None, :] - c[None, :, :]) ** 2).sum(2))                 # [tracks][proposals]
            t_idx, p_idx = np.nonzero(d <= gate)
            order = np.lexsort((p_idx, t_idx, d[t_idx, p_idx]))
            taken = np.zeros((len(last),), bool)
            for j in order:
                t, p = int(t_idx[j]), int(p_idx[j])
                if not taken[t] and mine[p] < 0:
                    taken[t], mine[p] = True, t
        for p in range(len(c)):
            if mine[p] < 0:
                mine[p] = len(tracks)
                tracks.append([])
                last.append(None)
            tracks[mine[p]].append((i, p))
            last[mine[p]] = c[p].copy()
        assigned.append(mine)
    return tracks, assigned


def best_views(loss, tracks_views):
    """int64 [T] on the device: per track the view (an index into `loss`) with the lowest loss -- the first on a tie, a NaN loses (all NaN:
    the first view).  tracks_views: per track the list of its views' indices (host); no synchronisation"""
    dev = loss.device
    n = max(len(v) for v in tracks_views)
    idx = np.array([list(v) + [v[0]] * (n - len(v)) for v in tracks_views], np.int64)
    pad = np.array([[0] * len(v) + [1] * (n - len(v)) for v in tracks_views], bool)
    idx_d, pad_d = _upload(torch.from_numpy(idx), dev), _upload(torch.from_numpy(pad), dev)
    ls = loss[idx_d]
    ls = torch.where(torch.isnan(ls) | pad_d, torch.full_like(ls, float("inf")), ls)
    pos = torch.arange(n, device=dev)[None, :].expand_as(ls)
    first = torch.where(ls == ls.min(1, keepdim=True).values, pos, torch.full_like(pos, n)).min(1).values
    return idx_d.gather(1, first[:, None])[:, 0]


def label_sequence(dsdf, grid, scans, K, w, h, world_to_cam, latent, cam_to_world=None, gate=2.0, cluster_kw=None, align_kw=None, joint_kw=None):
    """KITTI labels of several scans of one scene from the lidar and the shape prior `dsdf` alone, every object fitted ONCE over all its views.

    scans: a list of lidar clouds [N_i][3], each in its own camera frame; K, w, h: the camera; world_to_cam: the 4x4 p_WC of labels_many, one
    for all scans or one per scan; latent: the start latent of every proposal ([L]); cam_to_world: per scan the 4x4 that takes its camera
    frame to a common world frame (None: the identity -- a sensor at rest), used by the association alone; gate: metres, `associate`'s;
    cluster_kw, align_kw: keyword arguments of cluster.proposals and of the single-view align.align_many; joint_kw: those of
    track.align_tracks (origin, free_rows, eta, s_max and seed are NOT taken over from align_kw).  Steps:
      1. per scan frame.remove_road and cluster.proposals;
      2. ONE align_many batch over both yaw hypotheses of every proposal of every scan (rows 0 ... A - 1: yaw, rows A ... 2 A - 1: yaw + pi;
         proposals in scan order), and per proposal the hypothesis of the lower loss (scan.choose, on the device);
      3. `associate` on the host: the rectangle centres, taken to the world frame, into tracks;
      4. track.align_tracks from the chosen poses, the views of a track in scan order; a track starts from the latent and the scale of its
         view with the lowest single-view loss, chosen on the device (the first on a tie, a NaN loses);
      5. per scan frame.labels_many with the track's latent and scale and the view's yaw and trans; the 2-D boxes as in label_scan.
    HOST SYNCHRONISATIONS: S + 1 + sum_i ceil(A_i / 16) for S scans with A_i accepted proposals -- one per scan in proposals, one here (the
    2-D boxes and the choice, one copy), one per chunk of 16 annotations in each scan's labels_many; remove_road, align_many, the
    association and align_tracks make none.  Without any proposal it is the S of proposals.
    With one scan and joint_kw={'iters': 0} the labels are label_scan's in every bit.
    Returns (labels, stages): labels a list with one dict per scan in the shape frame.frame_dict makes, with the key 'track' (int64, the
    track of every label) added; stages = {'keep', 'proposals' (per scan), 'fits' (the Aligned of the 2 A-batch, or None), 'second',
    'tracks' and 'assigned' (associate's), 'joint' (the Tracked, or None), 'view' (per scan, per proposal its view's index in the joint fit),
    'params', 'bboxes', 'labels' (per scan)}."""
    scans = list(scans)
    S = len(scans)
    w2c = world_to_cam if isinstance(world_to_cam, (list, tuple)) else [world_to_cam] * S
    if len(w2c) != S or (cam_to_world is not None and len(cam_to_world) != S):
        raise ValueError("label_sequence: one world_to_cam and one cam_to_world per scan (%d scans)" % S)
    keeps = [FR.remove_road(lidar, K, w, h) for lidar in scans]
    props = [proposals(lidar, keep, latent=latent, **(cluster_kw or {})) for lidar, keep in zip(scans, keeps)]
    counts = [len(p) for p in props]
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)               # the first proposal of every scan in the batch
    A = int(first[-1])
    stages = {"keep": keeps, "proposals": props, "fits": None, "second": np.zeros(0, bool), "tracks": [], "assigned": [np.zeros(0, np.int64)] * S, "joint": None,
              "view": [np.zeros(0, np.int64)] * S, "params": [[] for _ in range(S)], "bboxes": [[] for _ in range(S)], "labels": [[] for _ in range(S)]}
    if A == 0:
        return [dict(FR.frame_dict([]), track=np.zeros(0, np.int64)) for _ in range(S)], stages
    starts = [q for p in props for q in p.params] + [q for p in props for q in p.flipped]
    clouds = [c for p in props for c in p.clouds]
    fits = align_many(dsdf, starts, clouds + clouds, **(align_kw or {}))
    second = choose(fits.loss, A)
    theta = torch.where(second[:, None], fits.theta[A:], fits.theta[:A])
    raw = torch.where(second[:, None], fits.raw_latents[A:], fits.raw_latents[:A])
    loss = torch.where(second, fits.loss[A:], fits.loss[:A])
    uv = torch.cat([pinhole_extents(p, K).reshape(-1) for p in props if len(p)])
    host = torch.cat([uv, second.float()]).cpu().numpy()                                 # the one host read of this function
    uv, sec = host[:4 * A].reshape(A, 4), host[4 * A:] != 0
    boxes = [np.array([np.clip(u0, 0, w), np.clip(v0, 0, h), np.clip(u1, 0, w), np.clip(v1, 0, h)], np.float32) for u0, u1, v0, v1 in uv]
    # association, on the host: the rectangles' centres in the world frame
    centres = []
    for i, p in enumerate(props):
        c = np.array([q["centre"] for q in p.info], np.float64).reshape(-1, 3)
        if cam_to_world is not None:
            M = np.asarray(cam_to_world[i].detach().cpu() if torch.is_tensor(cam_to_world[i]) else cam_to_world[i], np.float64).reshape(4, 4)
            c = c @ M[:3, :3].T + M[:3, 3]
        centres.append(c)
    tracks, assigned = associate(centres, gate)
    views = [[int(first[i]) + a for i, a in tr] for tr in tracks]                      # per track its views as rows of the batch, in scan order
    best = best_views(loss, views)
    z0, s0 = raw[best], theta[best, 4]
    joint = align_tracks(dsdf, [{"latent": z0[t], "scale": s0[t:t + 1],
                                 "views": [{"yaw": theta[a, 0:1], "trans": theta[a, 1:4], "cloud": clouds[a]} for a in views[t]]} for t in range(len(tracks))],
                         **(joint_kw or {}))
    view_of = {}
    for t, tr in enumerate(tracks):
        for j, key in enumerate(tr):
            view_of[key] = (t, j)
    labels = []
    for i in range(S):
        own = [view_of[(i, a)] for a in range(counts[i])]
        params = [joint.params[t][j] for t, j in own]
        bboxes = boxes[int(first[i]):int(first[i + 1])]
        labs = FR.labels_many(dsdf, grid, params, w2c[i], bboxes) if params else []
        out = FR.frame_dict(labs)
        out["track"] = np.array([t for (t, _), lab in zip(own, labs) if lab is not None], np.int64)
        labels.append(out)
        stages["view"][i] = np.array([joint.voff[t] + j for t, j in own], np.int64)
        stages["params"][i], stages["bboxes"][i], stages["labels"][i] = params, bboxes, labs
    stages.update(fits=fits, second=sec, tracks=tracks, assigned=assigned, joint=joint)
    return labels, stages
