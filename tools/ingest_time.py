"""GPU timing of frame ingest: depth_map, css_inputs_many, refine_sample and the road-plane removal.

depth_map     frame.depth_map of about 20 000 kept lidar points at 1242 x 375 (float64 cloud already on the device, and from the host).
css_inputs    frame.css_inputs_many on 1, 8 and 16 KITTI-sized boxes of one frame in one call against one call per box.
refine_sample pipelines.frame.refine_sample on the synthetic sample of fixtures.synthetic_sample against the path that existed before it: the
              depth map fetched to the host, the crops sliced in numpy, one css_inputs_many call and the same stand-in network, then
              refine_frame (the parent commit had no device code for the CSS input either; it is given the new kernel here, so the difference
              is the host slicing and the round trip alone).
road_removal  frame.remove_road and frame.kitti_frame on a synthetic velodyne-like scan of about 120 000 points of which about 20 000 fall into
              the 1242 x 375 frustum (scan and image already on the device), with their launches and host synchronisations.  Beside them the
              time of the same semantics on this machine's CPU: scipy.spatial.cKDTree.query(k=30, distance_upper_bound=1) over the frustum
              points and a batched numpy.linalg.eigh (frustum cut and depth map not included).  Open3D, which the reference calls, is not
              installed and cannot be timed; no threshold is set on any of these numbers.
launches      kernel launches and copies per call, counted with torch.profiler inside the sdfr:: ranges of _lib.traced; host
              synchronisations per call, counted with torch's sync debug mode.  The count refine_sample adds to refine_frame is printed.

One process, every timed call bounded by the caller's `timeout`; nothing is retried.  Host clock around calls that end in a synchronise,
the two sides alternating in the same run, median of REPS after WARM warm-up calls.

usage: python tools/ingest_time.py OUT_DIR          (writes OUT_DIR/ingest_time.json)
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sdflabel_amd  # noqa: E402
from frame_time import alternate, count_launches, count_syncs  # noqa: E402
from sdflabel_amd import frame as FR  # noqa: E402
from sdflabel_amd.fixtures import ASSET, stand_in_css, synthetic_sample  # noqa: E402
from sdflabel_amd.pipelines import optimizer as OP  # noqa: E402
from sdflabel_amd.pipelines import refinement as rtools  # noqa: E402
from sdflabel_amd.pipelines.frame import refine_frame, refine_sample  # noqa: E402

DEV = "cuda:0"


def counts(fn):
    k, c = count_launches(fn)
    return {"kernel_launches": k, "copies": c, "host_synchronisations": count_syncs(fn)}


def kitti_cloud(rng, n=26000, w=1242, h=375):
    K = np.array([[721.5377, 0, 609.5593], [0, 721.5377, 172.854], [0, 0, 1]], np.float64)
    z = rng.uniform(3.0, 70.0, n)
    u, v = rng.uniform(-150, w + 150, n), rng.uniform(-60, h + 60, n)
    v[::3] = rng.uniform(150, 260, len(v[::3]))
    u[::3] = rng.uniform(300, 700, len(u[::3]))
    return np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z], 1), K, w, h


def velodyne_scan(rng, beams=64, columns=2000):
    """A 360 degree scan in the camera frame (x right, y down, z forward), sensor 1.65 m above a flat road: every beam ends on the road or on an
    obstacle ring of random distance and height around the sensor; float32 values."""
    down = np.deg2rad(np.linspace(-2.0, 24.8, beams))[:, None]                       # the HDL-64E's elevations, positive = down
    az = np.linspace(-np.pi, np.pi, columns, endpoint=False)[None, :] + rng.uniform(0, 1e-3, (beams, 1))
    seg = rng.integers(0, 90, columns // 20 + 1)
    wall = np.repeat(np.where(seg < 55, rng.uniform(6.0, 60.0, len(seg)), 1e9), 20)[:columns][None, :]      # distance of the obstacle per column
    top = np.repeat(rng.uniform(1.2, 4.0, len(seg)), 20)[:columns][None, :]          # its height above the road
    with np.errstate(divide="ignore"):
        ground = np.where(down > 0, 1.65 / np.tan(np.maximum(down, 1e-9)), 1e9)
    r = np.minimum(ground, wall) * np.ones_like(az)
    y = r * np.tan(down)
    hit = (r < 120.0) & (y > 1.65 - top)
    r, y, a = r[hit] + rng.normal(0, 0.01, hit.sum()), y[hit] + rng.normal(0, 0.005, hit.sum()), (az * np.ones_like(down))[hit]
    pts = np.stack([r * np.sin(a), y, r * np.cos(a)], 1)
    return pts[rng.permutation(len(pts))].astype(np.float32).astype(np.float64)


def cpu_restatement_ms(pts, K, w, h, reps=3):
    """the neighbour search and the normals of the frustum points on the CPU: cKDTree and a batched eigh"""
    import time

    from scipy.spatial import cKDTree
    planes = FR.build_view_frustum(K, 0, 0, w, h).astype(np.float64)
    q = pts[(planes @ pts.T > 0).all(0)]
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dist, nn = cKDTree(q).query(q, k=30, distance_upper_bound=1.0)
        ok = np.isfinite(dist)
        nb = q[np.minimum(nn, len(q) - 1)]
        cnt = ok.sum(1)
        m = (nb * ok[:, :, None]).sum(1) / cnt[:, None]
        e = (nb - m[:, None]) * ok[:, :, None]
        C = np.einsum("nki,nkj->nij", e, e) / cnt[:, None, None]
        lam, V = np.linalg.eigh(C)
        road = (np.abs(V[:, 1, 0]) > 0.9) & (cnt >= 3)
        best.append((time.perf_counter() - t0) * 1e3)
    return {"frustum_points": int(len(q)), "road_points": int(road.sum()), "best_ms": round(min(best), 2), "runs_ms": [round(b, 2) for b in best]}


def road_removal(rng):
    K = np.array([[721.5377, 0, 609.5593], [0, 721.5377, 172.854], [0, 0, 1]], np.float64)
    w, h = 1242, 375
    scan = velodyne_scan(rng)
    scan_d = torch.from_numpy(scan).to(DEV)
    image_d = torch.from_numpy(rng.random((h, w, 3)).astype(np.float32)).to(DEV)
    keep, info = FR.remove_road(scan_d, K, w, h, return_info=True)
    inside = info["in_frustum"]
    cnt = info["nn_count"][inside]
    rr = lambda: FR.remove_road(scan_d, K, w, h)               # noqa: E731
    kf = lambda: FR.kitti_frame(image_d, scan_d, K)            # noqa: E731
    ta, tb = alternate(rr, kf)
    return {"scan_points": int(len(scan)), "frustum_points": int(inside.sum()), "kept_points": int(keep.sum()),
            "neighbourhoods_at_the_cap": int((cnt == 30).sum()), "neighbourhoods_below_3": int((cnt < 3).sum()), "image": [w, h],
            "remove_road": dict(ta, **counts(rr)), "kitti_frame": dict(tb, **counts(kf)),
            "cpu_restatement_ckdtree_eigh": cpu_restatement_ms(scan, K, w, h),
            "note": "scan and image on the device; Open3D is not installed and is not timed; no threshold"}


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.default_rng(19)
    res = {"config": "host clock around calls that end in a synchronise; the two sides alternate in the same run; median of 15 after 3 warm-up calls"}
    # the road-plane removal at KITTI size
    res["road_removal"] = road_removal(np.random.default_rng(23))
    print("road_removal", json.dumps(res["road_removal"]))
    # depth map
    lidar, K, w, h = kitti_cloud(rng)
    lidar_d = torch.from_numpy(lidar).to(DEV)
    on_dev = lambda: FR.depth_map(lidar_d, K, w, h)            # noqa: E731
    from_host = lambda: FR.depth_map(lidar, K, w, h)           # noqa: E731
    _, info = FR.depth_map(lidar_d, K, w, h, return_info=True)
    ta, tb = alternate(on_dev, from_host)
    res["depth_map"] = {"points": len(lidar), "points_on_a_pixel": int(info["counts"][0]), "image": [w, h], "cloud_on_the_device": dict(ta, **counts(on_dev)),
                        "cloud_from_the_host": dict(tb, **counts(from_host))}
    print("depth_map", json.dumps(res["depth_map"]))
    # CSS inputs
    image = torch.from_numpy(rng.random((h, w, 3)).astype(np.float32)).to(DEV)
    res["css_inputs"] = {}
    for A in (1, 8, 16):
        boxes = []
        for _ in range(A):
            bw = int(rng.integers(60, 420))
            bh = max(24, int(bw / rng.uniform(1.2, 3.2)))
            l, t = int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh))
            boxes.append([l, t, l + bw, t + bh])
        many = lambda: FR.css_inputs_many(image, boxes, orig=True)                          # noqa: E731
        loop = lambda: [FR.css_inputs_many(image, [b], orig=True) for b in boxes]           # noqa: E731
        tm, tl = alternate(many, loop)
        res["css_inputs"]["A%d" % A] = {"css_inputs_many": dict(tm, **counts(many)), "one_call_per_box": dict(tl, **counts(loop)),
                                        "crop_pixels": int(sum((b[2] - b[0]) * (b[3] - b[1]) for b in boxes))}
        print("css_inputs A=%d" % A, json.dumps(res["css_inputs"]["A%d" % A]))
    # refine_sample against the host-sliced composition
    dec32 = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV)
    dec16 = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float16)[0].to(DEV)
    grid = sdflabel_amd.Grid3D(40, DEV)
    sample, cloud = synthetic_sample(dec32, 40, 32, DEV)
    net = stand_in_css().to(DEV)
    W8, iters = {"2d": 0.3, "3d": 0.5}, 10
    annos = rtools.get_annos("", sample)
    boxes = [[int(v) for v in a["bbox"]] for a in annos]
    H, W = sample["image"].shape[:2]
    OP.clear_refiner_cache()

    def device_path():
        return refine_sample(sample, net, dec16, grid, iters, W8, lidar=cloud, seed=7)

    def host_path():
        depth = FR.depth_map(cloud, sample["orig_cam"], W, H).cpu().numpy()
        css_in = FR.css_inputs_many(sample["image"], boxes)
        with torch.no_grad():
            pred = net(css_in)
        annotations = [{"bbox": [l, t, r, b], "color": sample["image"][t:b, l:r].copy(), "depth": depth[t:b, l:r].copy(),
                        "nocs_pred": pred["uvw_sm_masked"][j] / 255.} for j, (l, t, r, b) in enumerate(boxes)]
        return refine_frame(annotations, dec16, grid, list(pred["latent"]), sample["orig_cam"], sample["world_to_cam"], iters, W8, seed=7)

    a, b = device_path(), host_path()
    same = all(a[0][k].tobytes() == b[0][k].tobytes() for k in FR.NECESSARY_KEYS)
    _, _, _, st = refine_sample(sample, net, dec16, grid, iters, W8, lidar=cloud, seed=7, return_stages=True)
    image_d = torch.from_numpy(sample["image"]).to(DEV)
    annotations = [{"bbox": bx, "color": image_d[bx[1]:bx[3], bx[0]:bx[2]], "depth": st["depth"][bx[1]:bx[3], bx[0]:bx[2]], "nocs_pred": st["nocs_pred"][j]}
                   for j, bx in enumerate(boxes)]
    frame_only = lambda: refine_frame(annotations, dec16, grid, st["latents"], sample["orig_cam"], sample["world_to_cam"], iters, W8, seed=7)   # noqa: E731
    det = np.stack([a_["bbox"] for a_ in annos]).astype(np.float32)
    labels = {"bboxes": torch.from_numpy(det), "masks": [torch.ones((int(b_ - t_), int(r_ - l_))) for l_, t_, r_, b_ in det]}
    masked = lambda: refine_sample(sample, net, dec16, grid, iters, W8, label_type="maskrcnn", maskrcnn_labels=labels, lidar=cloud, seed=7)   # noqa: E731
    frame_only(), masked()
    td, th = alternate(device_path, host_path)
    s_rf, s_gt, s_mr = count_syncs(frame_only), count_syncs(device_path), count_syncs(masked)
    res["refine_sample"] = {"annotations": len(annos), "kept": len(a[1]), "image": [W, H], "lidar_points": len(cloud), "iterations": iters,
                            "refine_sample": dict(td, **counts(device_path)), "host_sliced_composition": dict(th, **counts(host_path)),
                            "the_two_give_the_same_bits": bool(same),
                            "host_synchronisations": {"refine_frame": s_rf, "refine_sample_gt": s_gt, "refine_sample_maskrcnn": s_mr,
                                                      "added_by_refine_sample_gt": s_gt - s_rf, "added_by_refine_sample_maskrcnn": s_mr - s_rf}}
    print("refine_sample", json.dumps(res["refine_sample"]))
    print("host synchronisations added to refine_frame's %d: %d for label_type='gt', %d for 'maskrcnn'" % (s_rf, s_gt - s_rf, s_mr - s_rf))
    json.dump(res, open(os.path.join(out_dir, "ingest_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
