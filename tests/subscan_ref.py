"""Yardstick of the subscan-generation tests (csrc/visibility.hip, preprocessing/subscans.py), plain numpy only:

`visible_ref`   the frustum test in exactly the operation order the kernel promises (numpy never contracts a multiply and an add, so the
                kernel has to match it bit for bit);
`chain_ref`     the reference's own NumPy route to the camera frame -- homogeneous points times the transposed float32 world-to-camera
                matrix, one BLAS call whose summation order is not ours -- followed by the projection;
`walk_ref`      the reference's frame loop restated with bool arrays and `>=`;
`make_scan`     a synthetic scan: float32-valued points on the floor, the walls and furniture boxes of a room, cameras on a closed
                trajectory inside it with the yaw advancing frame by frame, so that consecutive frames overlap and a frame sees a sizeable
                share of the points.

The projection step of the reference is cv2.projectPoints with identity rotation, zero translation and zero distortion; OpenCV is not
installed here, so it is restated from the published implementation (multiply by the reciprocal of the depth, then x * fx + cx) and is not
pinned against an OpenCV build."""
import numpy as np

WIDTH, HEIGHT = 960.0, 540.0                       # the colour stream of a 3RScan sequence


def inverse_relative(pose):
    """World-to-camera from camera-to-world, as a FLOAT32 4x4 (the reference stores the inverse in a float32 array)."""
    pose = np.asarray(pose)
    rt = pose[:3, :3].T
    out = np.zeros((4, 4), dtype=np.float32)
    out[:3, :3] = rt
    out[:3, 3:4] = -np.dot(rt, pose[:3, 3:4])
    out[3, 3] = 1
    return out


def w2c_rows(poses):
    """[F, 4, 4] camera-to-world -> [F, 12] float64: rows 0-2 of the float32 world-to-camera matrices, widened."""
    return np.stack([inverse_relative(p)[:3].astype(np.float64).reshape(12) for p in poses]) if len(poses) else np.zeros((0, 12))


def make_intrinsics(fx=756.8, fy=756.0, cx=492.2, cy=270.4, width=WIDTH, height=HEIGHT):
    mat = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]).astype(np.float32)
    return {'width': float(width), 'height': float(height), 'intrinsic_mat': mat}


def intr_row(info):
    """fx, fy, cx, cy, u_max, v_max as float64.  The reference compares the FIRST image coordinate with the height and the second with
    the width; that is reproduced: u_max = height, v_max = width."""
    m = np.asarray(info['intrinsic_mat'])
    return np.array([m[0, 0], m[1, 1], m[0, 2], m[1, 2], info['height'], info['width']], dtype=np.float64)


def project_ref(pts, w2c12, intr):
    """One frame: (Z, u, v) float64 [N] in the promised operation order."""
    p = np.asarray(pts, dtype=np.float32).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    m = np.asarray(w2c12, dtype=np.float64).reshape(3, 4)
    fx, fy, cx, cy = (np.float64(v) for v in intr[:4])
    with np.errstate(all='ignore'):
        X = ((x * m[0, 0] + y * m[0, 1]) + z * m[0, 2]) + m[0, 3]
        Y = ((x * m[1, 0] + y * m[1, 1]) + z * m[1, 2]) + m[1, 3]
        Z = ((x * m[2, 0] + y * m[2, 1]) + z * m[2, 2]) + m[2, 3]
        r = np.where(Z != 0, 1.0 / np.where(Z != 0, Z, 1.0), 1.0)
        u = (X * r) * fx + cx
        v = (Y * r) * fy + cy
    return Z, u, v


def inside(Z, u, v, intr):
    with np.errstate(invalid='ignore'):
        return (Z > 0) & (u >= 0) & (u <= intr[4]) & (v >= 0) & (v <= intr[5])


def visible_ref(pts, w2c, intr):
    """pts [N, 3] float32, w2c [F, 12] float64, intr [6] float64 -> bool [F, N]."""
    out = np.zeros((len(w2c), len(pts)), dtype=bool)
    for f in range(len(w2c)):
        out[f] = inside(*project_ref(pts, w2c[f], intr), intr)
    return out


def near_threshold(Z, u, v, intr, rel=1e-9):
    """Entries within `rel` (relative to max(1, |value|)) of one of the five thresholds."""
    with np.errstate(invalid='ignore'):
        close = lambda a, t: np.abs(a - t) <= rel * np.maximum(1.0, np.abs(a))
        return close(Z, 0.0) | close(u, 0.0) | close(u, intr[4]) | close(v, 0.0) | close(v, intr[5])


def chain_ref(scene_pts, cam_2_world_pose, intrinsic_info):
    """The reference's route for one frame: bool [N]."""
    w2c = inverse_relative(cam_2_world_pose)
    homog = np.concatenate((scene_pts, np.ones((scene_pts.shape[0], 1), dtype=np.int64)), axis=1)
    cam = homog.dot(w2c.T)[..., :3]
    k = np.asarray(intrinsic_info['intrinsic_mat']).astype(np.float64)
    Z = cam[:, 2]
    with np.errstate(all='ignore'):
        r = np.where(Z != 0, 1.0 / np.where(Z != 0, Z, 1.0), 1.0)
        u = (cam[:, 0] * r) * k[0, 0] + k[0, 2]
        v = (cam[:, 1] * r) * k[1, 1] + k[1, 2]
        return (Z > 0.0) & ((u >= 0) & (u <= intrinsic_info['height'])) & ((v >= 0) & (v <= intrinsic_info['width']))


def walk_ref(masks, max_pts):
    """masks bool [F, N] -> dict(n_seg, seg_end [n_seg], seg_count [n_seg], frame_count [F], cum bool [F, N], seg_masks bool [n_seg, N])."""
    F, N = masks.shape
    cur = np.zeros(N, dtype=bool)
    seg_end, seg_count, frame_count, cum = [], [], np.zeros(F, dtype=np.int64), np.zeros((F, N), dtype=bool)
    for f in range(F):
        cur = np.logical_or(masks[f], cur)
        cum[f] = cur
        c = int(cur.sum())
        frame_count[f] = c
        if c >= max_pts:
            seg_end.append(f)
            seg_count.append(c)
            cur = np.zeros(N, dtype=bool)
    return {'n_seg': len(seg_end), 'seg_end': np.array(seg_end, dtype=np.int64), 'seg_count': np.array(seg_count, dtype=np.int64),
            'frame_count': frame_count, 'cum': cum, 'seg_masks': cum[seg_end] if seg_end else np.zeros((0, N), dtype=bool)}


def pack_bits(mask):
    """bool [..., N] -> uint64 [..., ceil(N / 64)]: bit p % 64 of word p / 64 is point p, padding bits 0."""
    mask = np.asarray(mask, dtype=bool)
    n = mask.shape[-1]
    w = (n + 63) // 64
    padded = np.zeros(mask.shape[:-1] + (w * 64,), dtype=np.uint8)
    padded[..., :n] = mask
    return np.packbits(padded, axis=-1, bitorder='little').view('<u8').reshape(mask.shape[:-1] + (w,))


ROOM = np.array([6.0, 4.5, 2.6])                   # metres; the room is [0, ROOM]
BOXES = (((0.4, 0.5, 0.0), (1.6, 1.3, 0.8)), ((4.2, 0.3, 0.0), (5.5, 1.0, 1.9)), ((2.2, 3.4, 0.0), (3.9, 4.2, 0.5)),
         ((0.3, 3.0, 0.0), (0.9, 4.1, 1.1)), ((4.8, 3.2, 0.0), (5.6, 4.0, 0.75)))


def _on_box(lo, hi, n, rng):
    """n points on the surface of an axis-aligned box (all six faces)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    p = lo + rng.random((n, 3)) * (hi - lo)
    axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    p[np.arange(n), axis] = np.where(side == 0, lo[axis], hi[axis])
    return p


def make_scan(n_points, n_frames, seed, blind=()):
    """-> dict(pts float32 [N, 3], object_id int16 [N], poses float64 [F, 4, 4] camera-to-world, intrinsics).  Object 1 is the floor, 2-5 the
    walls, 6.. the boxes.  The frames listed in `blind` are moved outside the room and look away from it: they see nothing."""
    rng = np.random.default_rng(seed)
    share = np.array([0.3, 0.1, 0.1, 0.1, 0.1] + [0.3 / len(BOXES)] * len(BOXES))
    obj = np.sort(rng.choice(len(share), size=n_points, p=share)) + 1
    pts = np.zeros((n_points, 3))
    for o in range(1, len(share) + 1):
        sel = np.flatnonzero(obj == o)
        m = len(sel)
        if o == 1:
            pts[sel] = np.column_stack([rng.random(m) * ROOM[0], rng.random(m) * ROOM[1], np.zeros(m)])
        elif o <= 5:
            a, h = rng.random(m), rng.random(m) * ROOM[2]
            pts[sel] = [np.column_stack([a * ROOM[0], np.zeros(m), h]), np.column_stack([a * ROOM[0], np.full(m, ROOM[1]), h]),
                        np.column_stack([np.zeros(m), a * ROOM[1], h]), np.column_stack([np.full(m, ROOM[0]), a * ROOM[1], h])][o - 2]
        else:
            pts[sel] = _on_box(*BOXES[o - 6], m, rng)
    order = rng.permutation(n_points) if n_points else np.zeros(0, dtype=np.int64)        # a ply does not store its vertices object by object
    pts, obj = pts[order].astype(np.float32), obj[order].astype(np.int16)
    poses = np.zeros((n_frames, 4, 4))
    t0, yaw0 = rng.random() * 2 * np.pi, rng.random() * 2 * np.pi
    for f in range(n_frames):
        t = t0 + 2 * np.pi * f / max(n_frames, 1)
        centre = np.array([ROOM[0] / 2 + 1.2 * np.cos(t), ROOM[1] / 2 + 0.8 * np.sin(t), 1.45 + 0.1 * np.sin(3 * t)])
        yaw = yaw0 + 0.21 * f
        fwd = np.array([np.cos(yaw), np.sin(yaw), -0.35 + 0.1 * np.sin(0.37 * f)])
        if f in blind:
            centre, fwd = np.array([60.0, 45.0, 1.45]), np.array([1.0, 1.0, 0.0])
        zc = fwd / np.linalg.norm(fwd)
        xc = np.cross(zc, [0.0, 0.0, 1.0])
        xc /= np.linalg.norm(xc)
        yc = np.cross(zc, xc)                                                            # x right, y down, z forward
        poses[f, :3, 0], poses[f, :3, 1], poses[f, :3, 2], poses[f, :3, 3], poses[f, 3, 3] = xc, yc, zc, centre, 1.0
    return {'pts': pts, 'object_id': obj, 'poses': poses, 'intrinsics': make_intrinsics()}


_CACHE = {}


def projected(scan):
    """(w2c [F, 12], intr [6], masks bool [F, N]) of a make_scan() dict, computed once per scan object and shared between tests."""
    key = id(scan)
    if key not in _CACHE:
        w2c, intr = w2c_rows(scan['poses']), intr_row(scan['intrinsics'])
        _CACHE[key] = (scan, w2c, intr, visible_ref(scan['pts'], w2c, intr))
    return _CACHE[key][1:]


def walk_cases():
    """The scans of the walk tests: dicts(scan, masks, max_pts).  Each closes at least two subscans and leaves a tail that is discarded,
    has a frame that sees nothing, and the second one's budget is met exactly by its first subscan (tests/test_subscans_cpu.py asserts all of it)."""
    if 'walk' not in _CACHE:
        cases = []
        for n, f, seed, frac, exact in ((1000, 33, 11, 0.2, False), (4097, 33, 12, 0.15, True), (20000, 40, 13, 0.2, False)):
            scan = make_scan(n, f, seed, blind=(5,))
            masks = projected(scan)[2]
            budget = int(frac * n)
            if exact:
                budget = int(walk_ref(masks, budget)['seg_count'][0])          # the first subscan closes at the same frame, now with c == max_pts
            cases.append({'scan': scan, 'masks': masks, 'max_pts': budget})
        _CACHE['walk'] = cases
    return _CACHE['walk']
