"""Synthetic bootstrap crops for the CSS network: posed shapes of the prior rendered into scenes, on the device (csrc/synth.hip; DESIGN.md
"Synthetic crops").

    from sdflabel_amd.synth import draw_scenes, scene_meshes, scenes_many

draw_scenes    host, float64, from a torch.Generator: which shapes stand where in each scene, their paint, the light and the background
scene_meshes   the scenes' shapes as lattice-frame meshes with decoder normals (mesh.meshes_many)
scenes_many    the scenes rendered: per object its NOCS image and its shaded colour crop, the scene's objects occluding each other

The method starts from a CSS network trained on renderings of the shape prior; this is a generator for such renderings.  It claims
nothing about the synthetic domain of the method's publication: one directional light, ambient + Lambert + Blinn-Phong, a colour ramp with
noise or a caller's image behind the cars.
"""
import math

import numpy as np
import torch

from . import _lib
from . import verify as _verify
from .export import Crop
from .mesh import meshes_many
from .pose import _upload
from .verify import _intrinsics

CUBE = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)], np.float64)


def _uniform(g, lo, hi):
    return float(lo) + (float(hi) - float(lo)) * float(torch.rand((), generator=g, dtype=torch.float64))


def _cam_T(yaw, trans, scale):
    """frame.assemble_labels' cam_T for float32 (yaw, trans, scale) and an identity world_to_cam: what meshes_many sets on the mesh"""
    from .frame import assemble_labels
    _, T = assemble_labels(np.zeros((1, 6), np.float32), np.asarray([yaw], np.float32), np.asarray(trans, np.float32).reshape(1, 3),
                           np.asarray([scale], np.float32), np.eye(4), [None])
    return T[0]


def _cube_corners(cam_T, scale):
    """the 8 corners of the lattice cube [-1, 1]^3 in the camera frame, float64 [8][3]"""
    return (CUBE * float(scale)) @ cam_T[:3, :3].T + cam_T[:3, 3]


def _scene_seed(seed, index):
    """a 63-bit seed of scene `index` from the generator's seed (splitmix64 finaliser, pose.py)"""
    from .pose import _mix64
    with np.errstate(over="ignore"):
        u = np.uint64
        z = _mix64(u(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ _mix64(u(int(index) & 0xFFFFFFFFFFFFFFFF) * u(0x9E3779B97F4A7C15) + u(1)))
    return int(z) >> 1


def draw_scenes(generator, n_scenes, n_latents, K, image_size, first_scene=0, max_objects=3, scale_range=(1.4, 2.4), z_near=8.0, z_far=40.0,
                border=0.05, blend=0.5, albedo_range=(0.1, 0.9), ks_range=(0.0, 0.5), shin_range=(2, 6), ambient_range=(0.15, 0.4),
                kd_range=(0.5, 0.9), jitter=0.1, noise_range=(0, 48), n_backgrounds=0, z_min=0.1):
    """Draw scenes first_scene .. first_scene + n_scenes - 1 on the host, in float64.

    A SCENE DEPENDS ON (generator.initial_seed(), scene index) ONLY: every scene draws from a generator of its own seeded by the two, so
    the same scene comes out whatever n_scenes, first_scene or the generator's state are.  Per scene: 1 .. max_objects objects; the light
    'light' (a unit vector of the camera frame pointing from the surface towards the light, in the upper hemisphere -- y < 0 -- and on the
    camera's side, z < 0), 'ambient', 'kd'; 'background' (an index below n_backgrounds, or None for the procedural one) and 'ramp' (top and
    bottom colour, noise amplitude from noise_range, noise seed).  Per object: 'latent' (an index below n_latents) or, with probability
    `blend`, 'latent' = (i0, i1, w) for (1 - w) latents[i0] + w latents[i1]; 'yaw' uniform in [-pi, pi); 'scale' in scale_range; the depth
    'z' uniform in [z_near, z_far]; the projected centre 'u', 'v' uniform in the image inset by `border` of its width / height, and
    'trans' = z K^-1 (u, v, 1) / scale, so that the label's translation trans * scale puts the centre there: every object's centre is inside
    the image; 'albedo', 'ks', 'shin' (the specular exponent is 2^shin); 'jitter', four fractions in [-jitter, jitter] by which scenes_many
    moves the sides of the crop's box.  An object with a corner of its lattice cube at Z <= z_min is drawn again (ValueError after 64
    tries: the ranges leave no room).

    ALL RANGES ARE PARAMETERS AND THE DEFAULTS CLAIM NO OPERATING POINT: the method's published synthetic domain is not reproduced, and
    nothing here was tuned against a trained network."""
    fx, fy, cx, cy = _intrinsics(K)
    W, H = int(image_size[0]), int(image_size[1])
    if n_latents < 1 or max_objects < 1 or not 0.0 <= float(border) < 0.5 or not float(z_near) > float(z_min):
        raise ValueError("draw_scenes: needs n_latents >= 1, max_objects >= 1, 0 <= border < 0.5 and z_near > z_min")
    seed = generator.initial_seed()
    scenes = []
    for index in range(int(first_scene), int(first_scene) + int(n_scenes)):
        g = torch.Generator().manual_seed(_scene_seed(seed, index))
        n_obj = int(torch.randint(1, int(max_objects) + 1, (), generator=g))
        lx, ly, lz = _uniform(g, -1.0, 1.0), _uniform(g, -1.0, -0.2), _uniform(g, -1.0, -0.2)
        ln = math.sqrt(lx * lx + ly * ly + lz * lz)
        sc = {'index': index, 'light': [lx / ln, ly / ln, lz / ln], 'ambient': _uniform(g, *ambient_range), 'kd': _uniform(g, *kd_range),
              'background': int(torch.randint(0, int(n_backgrounds), (), generator=g)) if n_backgrounds > 0 else None,
              'ramp': [int(x) for x in torch.randint(0, 256, (6,), generator=g)] +
                      [int(torch.randint(int(noise_range[0]), int(noise_range[1]) + 1, (), generator=g)),
                       int(torch.randint(0, 2 ** 31 - 1, (), generator=g))],
              'objects': []}
        for _ in range(n_obj):
            for attempt in range(64):
                o = {}
                i0 = int(torch.randint(0, int(n_latents), (), generator=g))
                if _uniform(g, 0.0, 1.0) < float(blend) and n_latents > 1:
                    o['latent'] = (i0, int(torch.randint(0, int(n_latents), (), generator=g)), _uniform(g, 0.0, 1.0))
                else:
                    o['latent'] = i0
                o['yaw'] = _uniform(g, -math.pi, math.pi)
                o['scale'] = _uniform(g, *scale_range)
                o['z'] = _uniform(g, z_near, z_far)
                o['u'] = _uniform(g, float(border) * W, (1.0 - float(border)) * W)
                o['v'] = _uniform(g, float(border) * H, (1.0 - float(border)) * H)
                centre = np.array([(o['u'] - cx) / fx * o['z'], (o['v'] - cy) / fy * o['z'], o['z']], np.float64)
                o['trans'] = (centre / o['scale']).tolist()
                o['albedo'] = [_uniform(g, *albedo_range) for _ in range(3)]
                o['ks'] = _uniform(g, *ks_range)
                o['shin'] = int(torch.randint(int(shin_range[0]), int(shin_range[1]) + 1, (), generator=g))
                o['jitter'] = [_uniform(g, -float(jitter), float(jitter)) for _ in range(4)]
                T = _cam_T(o['yaw'], o['trans'], o['scale'])
                if _cube_corners(T, np.float32(o['scale']))[:, 2].min() > float(z_min):
                    break
            else:
                raise ValueError("draw_scenes: no object with its lattice cube beyond z_min = %g in 64 tries (scale %s, depth %g .. %g)"
                                 % (z_min, tuple(scale_range), z_near, z_far))
            sc['objects'].append(o)
        scenes.append(sc)
    return scenes


def _objects(scenes):
    return [(si, oi, o) for si, s in enumerate(scenes) for oi, o in enumerate(s['objects'])]


def _latent_rows(latents, objs, dev):
    """float32 [B][L] on the device: the raw latent every object is decoded from (a row, or the blend of two); no host read"""
    lat = latents.detach() if torch.is_tensor(latents) else torch.as_tensor(np.asarray(latents))
    lat = lat.to(torch.float32).reshape(lat.shape[0], -1)
    lat = lat.to(dev) if lat.is_cuda else _upload(lat.contiguous(), dev)
    rows = []
    for _, _, o in objs:
        sel = o['latent']
        if isinstance(sel, (tuple, list)):
            i0, i1, w = int(sel[0]), int(sel[1]), float(sel[2])
            rows.append(lat[i0] * (1.0 - w) + lat[i1] * w)
        else:
            rows.append(lat[int(sel)])
    return torch.stack(rows).contiguous()


def scene_meshes(dsdf, latents, scenes, resolution=64):
    """The camera-frame meshes (Mesh.to_camera(): decoder normals, .lattice_vertices, .scale and .cam_T set) of all objects of all scenes, in
    scene order, and the raw latents [B][L] they were decoded from.  mesh.meshes_many's launches and host reads."""
    objs = _objects(scenes)
    dev = next(dsdf.parameters()).device
    if not objs:
        return [], torch.zeros((0, int(dsdf.latent_size)), device=dev)
    rows = _latent_rows(latents, objs, dev)
    shapes = [{'latent': rows[b], 'yaw': np.float32(o['yaw']), 'trans': np.asarray(o['trans'], np.float32), 'scale': np.float32(o['scale'])}
              for b, (_, _, o) in enumerate(objs)]
    return [m.to_camera() for m in meshes_many(dsdf, shapes, resolution=resolution, polish=True, normals=True)], rows


def cube_window(cam_T, scale, K, image_size, z_min=0.1):
    """the window [l, t, r, b) of an object without a device read: the 8 corners of the lattice cube through scale, cam_T and K in float64,
    rounded outward, grown by one pixel, clipped to the image.  A corner at Z <= z_min raises."""
    fx, fy, cx, cy = _intrinsics(K)
    W, H = int(image_size[0]), int(image_size[1])
    c = _cube_corners(np.asarray(cam_T, np.float64), scale)
    if not c[:, 2].min() > float(z_min):
        raise ValueError("synth: a corner of the object's lattice cube lies at Z = %g <= z_min = %g" % (c[:, 2].min(), z_min))
    u, v = fx * c[:, 0] / c[:, 2] + cx, fy * c[:, 1] / c[:, 2] + cy
    l, t, r, b = math.floor(u.min()) - 1, math.floor(v.min()) - 1, math.ceil(u.max()) + 2, math.ceil(v.max()) + 2
    l, t, r, b = min(max(l, 0), W), min(max(t, 0), H), min(max(r, 0), W), min(max(b, 0), H)
    return l, t, max(r, l), max(b, t)


def jittered_box(tight, jitter, window):
    """the crop's box: the tight box of the covered pixels with its sides moved by jitter (l, t, r, b fractions of its width / height,
    positive = outward; rounded half to even), clipped to the window; never smaller than one pixel of the tight box"""
    l, t, r, b = (int(x) for x in tight)
    w, h = r - l, b - t
    l2, t2 = l - int(round(jitter[0] * w)), t - int(round(jitter[1] * h))
    r2, b2 = r + int(round(jitter[2] * w)), b + int(round(jitter[3] * h))
    l2, t2, r2, b2 = max(l2, window[0]), max(t2, window[1]), min(r2, window[2]), min(b2, window[3])
    if r2 <= l2:
        l2, r2 = l, r
    if b2 <= t2:
        t2, b2 = t, b
    return l2, t2, r2, b2


@_lib.traced("scenes_many")
def scenes_many(dsdf, latents, scenes, K, image_size, resolution=64, z_min=0.1, min_pixels=16, backgrounds=None, meshes=None, _launches=None):
    """Render draw_scenes' scenes: per object a Crop with `.uvw` (NOCS bytes, as export.crops_many's) and `.rgb` (the shaded colour image of
    the crop's box: the scene's objects where they are in sight, its background elsewhere).

    latents: [n][L], the rows the scenes' latent indices refer to.  K, image_size: shared by all scenes -- they are different images of one
    camera.  backgrounds: uint8 [n][H][W][3] RGB images (device or host) for the scenes' 'background' indices; None: every scene shows its
    procedural ramp.  meshes: scene_meshes(dsdf, latents, scenes, resolution) made beforehand (meshes, latent rows); None: made here, and
    mesh.meshes_many's host reads add to the one below.

    1. scene_meshes: the meshes with decoder normals, posed by frame.assemble_labels' cam_T for the drawn float32 (yaw, trans, scale) and
       taken to the camera frame (Mesh.to_camera())
    2. every object's window from its lattice cube's corners on the host (cube_window)
    3. verify.raster_batch, RasterBatch.mask_counts and THE ONE HOST READ of the call, [B][8]: the crop's box is the tight box of the covered
       pixels moved by the drawn jitter and clipped to the window (jittered_box); an object that covers fewer than min_pixels pixels
       (before occlusion) gets no crop but stays in its scene as an occluder
    4. sdfr_synth_owner (an object is occluded by the objects of its own scene only), sdfr_crop_export, sdfr_synth_shade, sdfr_crop_counts

    Returns (crops, report): export.Crop objects with `.latent` (the raw latent decoded), `.intrinsics` (K), `.extrinsics` (cam_T), `.scene`
    (the scene's 'index'), `.object` and `.yaw` filled in; report = {'kept': [(scene, object)], 'dropped': [(scene, object)], 'area':
    covered pixels per object}.  A crop's bytes depend on its own scene only, not on the scenes that share the call.  The same bits on every
    run."""
    L = _lib.lib()
    objs = _objects(scenes)
    B, S = len(objs), len(scenes)
    W, H = int(image_size[0]), int(image_size[1])
    report = {'kept': [], 'dropped': [], 'area': []}
    if B == 0:
        return [], report
    if meshes is None:
        meshes = scene_meshes(dsdf, latents, scenes, resolution)
    cam, rows = meshes
    if len(cam) != B:
        raise ValueError("scenes_many: %d meshes for %d objects" % (len(cam), B))
    for b, m in enumerate(cam):
        if m.normals is None:
            raise ValueError("scenes_many: mesh %d has no normals (meshes_many(normals=True))" % b)
        if m.frame != "camera" or m.lattice_vertices is None or m.scale is None or m.cam_T is None:
            raise ValueError("scenes_many: mesh %d is not a camera-frame mesh made by Mesh.to_camera() with scale and cam_T" % b)
    win = np.array([cube_window(m.cam_T, m.scale, K, image_size, z_min) for m in cam], np.int64).reshape(B, 4)
    rb = _verify.raster_batch(cam, K, win, image_size, z_min)
    dev = rb.device
    c8 = rb.mask_counts().cpu().numpy().astype(np.int64)                                  # the one host read
    box = np.zeros((B, 4), np.int64)
    for b, (si, oi, o) in enumerate(objs):
        area = int(c8[b, 0])
        report['area'].append(area)
        if area < max(int(min_pixels), 1) or (c8[b, 7] & _verify.FLAG_INVALID):
            report['dropped'].append((scenes[si]['index'], oi))
            box[b] = [win[b, 0], win[b, 1], win[b, 0], win[b, 1]]                        # an empty box inside the window: no pixels
        else:
            report['kept'].append((scenes[si]['index'], oi))
            box[b] = jittered_box(c8[b, 1:5], o['jitter'], win[b])
    qoff = np.concatenate([[0], np.cumsum((box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1]))]).astype(np.int64)
    Q, P = int(qoff[-1]), rb.P
    scene_of = np.array([si for si, _, _ in objs], np.int32)
    ints = np.concatenate([box.astype(np.int32).reshape(-1), scene_of,
                           np.array([-1 if s.get('background') is None else int(s['background']) for s in scenes], np.int32),
                           np.array([s['ramp'] for s in scenes], np.int32).reshape(-1)])
    ints = np.concatenate([ints, np.zeros(len(ints) % 2, np.int32)])
    dbl = np.concatenate([np.array([list(o['albedo']) + [o['ks'], o['shin']] for _, _, o in objs], np.float64).reshape(-1),
                          np.array([list(s['light']) + [s['ambient'], s['kd']] for s in scenes], np.float64).reshape(-1)])
    table = _upload(torch.from_numpy(np.concatenate([qoff, ints.view(np.int64), dbl.view(np.int64)])), dev)
    d_qoff = table[:B + 1]
    d_int = table[B + 1:B + 1 + len(ints) // 2].view(torch.int32)
    d_dbl = table[B + 1 + len(ints) // 2:].view(torch.float64)
    d_box, d_scene, d_bgi, d_ramp = d_int[:4 * B], d_int[4 * B:5 * B], d_int[5 * B:5 * B + S], d_int[5 * B + S:5 * B + 9 * S]
    d_paint, d_light = d_dbl[:5 * B], d_dbl[5 * B:]
    bg, NBG = None, 0
    if backgrounds is not None:
        bg = backgrounds.detach() if torch.is_tensor(backgrounds) else torch.from_numpy(np.ascontiguousarray(backgrounds))
        if bg.dtype != torch.uint8 or bg.dim() != 4 or tuple(bg.shape[1:]) != (H, W, 3):
            raise ValueError("scenes_many: backgrounds must be uint8 [n][%d][%d][3], got %s %s" % (H, W, bg.dtype, tuple(bg.shape)))
        bg = (bg if bg.is_cuda else _upload(bg, dev)).contiguous()
        NBG = int(bg.shape[0])
    attr = torch.cat([m.lattice_vertices.detach().to(torch.float32).reshape(-1, 3) for m in cam]).contiguous()
    nrm = torch.cat([m.normals.detach().to(torch.float32).reshape(-1, 3) for m in cam]).contiguous()
    uvw = torch.empty((Q, 3), dtype=torch.uint8, device=dev)
    rgb = torch.empty((Q, 3), dtype=torch.uint8, device=dev)
    owner = torch.empty((P,), dtype=torch.int32, device=dev)
    flags = torch.empty((2, B), dtype=torch.int32, device=dev)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    Pt, ck = _lib.ptr, _lib.check
    V, T = int(rb.vertices.shape[0]), int(rb.faces.shape[0])
    mesh_args = (Pt(rb.vertices) if V else None, V, Pt(rb.faces) if T else None, T)

    def run_owner():
        with _lib.guard(dev):
            ck(L.sdfr_synth_owner(Pt(rb.mask) if P else None, Pt(rb.depth) if P else None, Pt(rb.d_win), Pt(rb.d_poff), P, Pt(d_scene), B, W, H,
                                  Pt(owner) if P else None, _lib.stream_ptr()), "sdfr_synth_owner")

    def run_shade():
        with _lib.guard(dev):
            ck(L.sdfr_synth_shade(*mesh_args, Pt(nrm) if V else None, Pt(rb.d_voff), Pt(rb.d_toff), Pt(rb.d_win), Pt(rb.d_poff), P,
                                  Pt(rb.triangle) if P else None, Pt(owner) if P else None, Pt(d_scene), Pt(d_box), Pt(d_qoff), Q, Pt(d_paint),
                                  Pt(d_light), S, Pt(d_bgi), Pt(bg), NBG, Pt(d_ramp), B, W, H, rb.k4, float(z_min), Pt(rgb) if Q else None, Pt(flags[1]),
                                  _lib.stream_ptr()), "sdfr_synth_shade")

    run_owner()
    with _lib.guard(dev):
        st = _lib.stream_ptr()
        ck(L.sdfr_crop_export(*mesh_args, Pt(attr) if V else None, Pt(rb.d_voff), Pt(rb.d_toff), Pt(rb.d_win), Pt(rb.d_poff), P,
                              Pt(rb.triangle) if P else None, Pt(owner) if P else None, Pt(d_box), Pt(d_qoff), Q, None, B, W, H, rb.k4, float(z_min),
                              Pt(uvw) if Q else None, None, Pt(flags[0]), st), "sdfr_crop_export")
    run_shade()
    with _lib.guard(dev):
        ck(L.sdfr_crop_counts(Pt(rb.mask) if P else None, Pt(owner) if P else None, Pt(rb.d_win), Pt(rb.d_poff), P, Pt(d_box), Pt(d_qoff), Q,
                              Pt(flags[0]), B, W, H, Pt(counts), _lib.stream_ptr()), "sdfr_crop_counts")
    if _launches is not None:                                # tools/synth_time.py: the two new entry points again, on the same buffers
        _launches.update(owner=run_owner, shade=run_shade, window_pixels=P, box_pixels=Q)
    word = counts[:, 3] | flags[1] | rb.flags
    k3 = np.array([[_intrinsics(K)[0], 0.0, _intrinsics(K)[2]], [0.0, _intrinsics(K)[1], _intrinsics(K)[3]], [0.0, 0.0, 1.0]])
    dropped = set(report['dropped'])
    out = []
    for b, (si, oi, o) in enumerate(objs):
        if (scenes[si]['index'], oi) in dropped:
            continue
        l, t, r, bt = (int(x) for x in box[b])
        q0, q1 = int(qoff[b]), int(qoff[b + 1])
        shape = (bt - t, r - l, 3)
        c = Crop(uvw[q0:q1].view(shape), rgb[q0:q1].view(shape), (l, t, r, bt), tuple(int(x) for x in win[b]), counts[b], word[b],
                 latent=rows[b], intrinsics=k3, extrinsics=np.asarray(cam[b].cam_T, np.float64))
        c.scene, c.object, c.yaw = scenes[si]['index'], oi, float(o['yaw'])
        out.append(c)
    return out, report
