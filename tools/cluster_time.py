"""GPU timing of the lidar clusters and rough boxes (csrc/cluster.hip, sdflabel_amd/cluster.py, pipelines/scan.py).

inputs      tests/_normals_ref.street(1) (about 2 400 points) and the KITTI-sized synthetic scan of tools/ingest_time.py (119 260 points, about
            15 000 in the 1242 x 375 frustum), road removed by frame.remove_road first; the mask and the scan are on the device.
clusters    cluster.clusters alone; boxes: cluster.boxes alone on its result; proposals: both with the one host read and the host arithmetic.
label_scan  pipelines.scan.label_scan with the asset decoder on the scan (whose walls the gates reject: it ends after the proposals) and on the
            planted scene of the tests (three objects), there with its stages one by one (proposals, align_many on both hypotheses,
            labels_many).  clusters_of_every_frustum_point: clusters with the frustum cut alone as the mask.
launches    kernel launches and copies per call (torch.profiler), host synchronisations per call (torch's sync debug mode).
cpu         the same semantics on this machine's CPU: scipy.spatial.cKDTree pairs within eps of the kept points and
            scipy.sparse.csgraph.connected_components; query_pairs (one thread: it has no worker option) and query_ball_point with 16 workers.

Device events around windows of CALLS back-to-back calls for the calls without a host synchronisation, the median of REPS windows after WARM
warm-up windows; the host clock around single calls for those that end in a host read.  No ratio is fixed in advance; the figures to read
against are the CPU time of the same run and remove_road's time (profiles/ingest_time.json).

usage: python tools/cluster_time.py OUT_DIR         (writes OUT_DIR/cluster_time.json)
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sdflabel_amd  # noqa: E402
from frame_time import count_launches, count_syncs  # noqa: E402
from ingest_time import velodyne_scan  # noqa: E402
from sdflabel_amd import cluster as C  # noqa: E402
from sdflabel_amd import frame as FR  # noqa: E402
from sdflabel_amd.align import align_many  # noqa: E402
from sdflabel_amd.fixtures import ASSET  # noqa: E402
from sdflabel_amd.pipelines import scan  # noqa: E402

DEV = "cuda:0"
CALLS, WARM, REPS = 20, 2, 9
K = np.array([[721.5377, 0, 609.5593], [0, 721.5377, 172.854], [0, 0, 1]], np.float64)
W, H = 1242, 375
ALIGN = dict(iters=60, rows_per_iter=512, lr_step=40)


def stat(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def windows(fn):
    """device events around CALLS back-to-back calls: per-call milliseconds, median of REPS windows"""
    out = []
    for r in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        b.synchronize()
        if r >= WARM:
            out.append(a.elapsed_time(b) / CALLS)
    return stat(out)


def host_clock(fn, reps=REPS, warm=WARM):
    out = []
    for r in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return stat(out)


def counts(fn):
    k, c = count_launches(fn)
    return {"kernel_launches": k, "copies": c, "host_synchronisations": count_syncs(fn)}


def cpu_ms(pts, eps, reps=3):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    n = len(pts)
    one, many, comps = [], [], 0
    for _ in range(reps):
        t0 = time.perf_counter()
        pr = cKDTree(pts).query_pairs(eps, output_type="ndarray")
        comps, _ = connected_components(coo_matrix((np.ones(len(pr), np.int8), (pr[:, 0], pr[:, 1])), shape=(n, n)), directed=False)
        one.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        nb = cKDTree(pts).query_ball_point(pts, eps, workers=16)
        lens = np.fromiter((len(x) for x in nb), np.int64, n)
        g = coo_matrix((np.ones(int(lens.sum()), np.int8), (np.repeat(np.arange(n), lens), np.concatenate(nb).astype(np.int64))), shape=(n, n))
        comps2, _ = connected_components(g, directed=False)
        many.append((time.perf_counter() - t0) * 1e3)
        assert comps2 == comps
    return {"points": n, "components": int(comps), "query_pairs_one_thread": stat(one), "query_ball_point_16_workers": stat(many)}


def frustum_only(pts, kw):
    """clusters with the frustum cut alone as the mask (the road stays in: one large component), the most points this input can give"""
    _, info = FR.lidar_normals(pts, K, W, H, return_info=True)
    inside = info["in_frustum"]
    f = lambda: C.clusters(pts, inside, **kw)                       # noqa: E731
    return dict(windows(f), participating=int(inside.sum()), counts=[int(v) for v in f().counts.cpu()])


def one_input(name, pts_host, eps, min_points):
    pts = torch.from_numpy(pts_host).to(DEV)
    keep = FR.remove_road(pts, K, W, H)
    lat = torch.tensor([0.3, -0.5, 0.8], device=DEV)
    kw = dict(eps=eps, min_points=min_points)
    cl = C.clusters(pts, keep, **kw)
    f_cl = lambda: C.clusters(pts, keep, **kw)                      # noqa: E731
    f_bx = lambda: C.boxes(None, cl)                                # noqa: E731
    f_pr = lambda: C.proposals(pts, keep, latent=lat, **kw)         # noqa: E731
    f_rr = lambda: FR.remove_road(pts, K, W, H)                     # noqa: E731
    props = f_pr()
    res = {"points": int(len(pts_host)), "kept_points": int(keep.sum()), "eps": eps, "min_points": min_points,
           "counts": [int(v) for v in props.counts], "accepted": len(props),
           "remove_road": dict(windows(f_rr), **counts(f_rr)),
           "clusters": dict(windows(f_cl), **counts(f_cl)),
           "boxes": dict(windows(f_bx), **counts(f_bx)),
           "proposals": dict(host_clock(f_pr), **counts(f_pr)),
           "clusters_of_every_frustum_point": frustum_only(pts, kw),
           "cpu_ckdtree_connected_components": cpu_ms(pts_host[keep.cpu().numpy()], eps)}
    print(name, json.dumps(res))
    return res, pts, keep, lat


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    from tests import _normals_ref as NR
    res = {"config": "device events around windows of %d calls, median of %d windows after %d warm-up (remove_road, clusters, boxes); host clock "
                     "around single calls that end in a host read (proposals, label_scan and its stages), median of %d after %d" % (CALLS, REPS, WARM, REPS, WARM),
           "device": torch.cuda.get_device_name(0), "form": "one wave per sorted slot (the thread-per-point form was not built)"}
    res["street"], _, _, _ = one_input("street", NR.street(1), 0.5, 10)
    res["kitti_sized_scan"], pts, keep, lat = one_input("kitti_sized_scan", velodyne_scan(np.random.default_rng(23)), 0.5, 10)
    # label_scan and its stages
    dec = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV).eval()
    grid = sdflabel_amd.Grid3D(40, DEV)
    p_WC = np.eye(4)
    f_ls = lambda: scan.label_scan(dec, grid, pts, K, W, H, p_WC, lat, align_kw=ALIGN)       # noqa: E731
    est, st = f_ls()
    props = st["proposals"]
    A = len(props)
    ls = {"proposals": A, "labels": len(est["name"]), "align": ALIGN, "label_scan": dict(host_clock(f_ls, 5, 1), **counts(f_ls))}
    if A:
        f_al = lambda: align_many(dec, props.params + props.flipped, props.clouds + props.clouds, **ALIGN)       # noqa: E731
        f_lb = lambda: FR.labels_many(dec, grid, st["params"], p_WC, st["bboxes"])                                # noqa: E731
        ls["stages"] = {"remove_road": res["kitti_sized_scan"]["remove_road"], "proposals": res["kitti_sized_scan"]["proposals"],
                        "align_many_both_hypotheses": dict(host_clock(f_al, 5, 1), **counts(f_al)),
                        "labels_many": dict(host_clock(f_lb, 5, 1), **counts(f_lb))}
    res["label_scan"] = ls
    print("label_scan", json.dumps(ls))
    # the planted scene of the tests (three objects; its road-free points, every one taking part): label_scan and its stages
    from tests import _cluster_ref as CR
    sc, s = CR.planted_scene(), CR.SCENE
    pp = torch.from_numpy(np.array(sc["points"][sc["mask"] != 0])).to(DEV)
    zl = torch.from_numpy(np.array(sc["z_true"])).to(DEV)
    ckw = dict(eps=s["eps"], min_points=s["min_points"], max_clusters=64, n_angles=s["n_angles"], scale=s["scale"], gates=s["gates"])
    f_ps = lambda: scan.label_scan(dec, grid, pp, K, W, H, p_WC, zl, remove_road=False, cluster_kw=ckw, align_kw=ALIGN)       # noqa: E731
    est, st = f_ps()
    props = st["proposals"]
    f_pr = lambda: C.proposals(pp, None, latent=zl, **ckw)                                                        # noqa: E731
    f_al = lambda: align_many(dec, props.params + props.flipped, props.clouds + props.clouds, **ALIGN)            # noqa: E731
    f_lb = lambda: FR.labels_many(dec, grid, st["params"], p_WC, st["bboxes"])                                    # noqa: E731
    res["planted_scene"] = {"points": int(len(pp)), "proposals": len(props), "labels": len(est["name"]), "align": ALIGN,
                            "label_scan": dict(host_clock(f_ps, 5, 1), **counts(f_ps)),
                            "stages": {"proposals": dict(host_clock(f_pr, 5, 1), **counts(f_pr)),
                                       "align_many_both_hypotheses": dict(host_clock(f_al, 5, 1), **counts(f_al)),
                                       "labels_many": dict(host_clock(f_lb, 5, 1), **counts(f_lb))}}
    print("planted_scene", json.dumps(res["planted_scene"]))
    json.dump(res, open(os.path.join(out_dir, "cluster_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
