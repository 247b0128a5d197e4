"""The survey attitude rule (include/wm_hip.h "Survey attitude") restated for the tests, the cases they share, the mutants that
show the cases have teeth, and a closed-form forward model of a tilted camera over flat ground with the two-frame census
scene built on it.  The rule has no reference behaviour: attitude_oracle is its restatement in numpy float64, the header's
expression statement for statement -- elementwise numpy arithmetic is one correctly rounded IEEE operation per element and
operator -- and the device must equal it byte for byte.  The inside test and the sampling are the ground rules'
(ground_oracle: inside, _sample_many), imported, not restated; cameras, the fill and the shapes are lens_cases'.

The host layer under test (wildlifemapper_amd.attitude) is used only to turn (roll, pitch) into a matrix and keep='valid' /
keep='all' into a size; every expected byte comes from attitude_oracle.  Nothing here asserts."""
import functools

import numpy as np

from ground_oracle import _sample_many, inside
from lens_cases import BARREL, FILL, FIVE, MODES, OUT_HEIGHTS, OUT_WIDTHS, SOURCE_SIZES, _spanning, camera  # noqa: F401

F64 = np.float64
IDENTITY = np.eye(3)
QUARTER = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])

MUTANTS = ("rot_transposed", "roll_flipped", "pitch_flipped", "z_test_dropped", "z_division_dropped", "r2_r5_dropped", "lens_before_rotation")


def rotation(roll=0.0, pitch=0.0, turn=0.0):
    """rot of roll and pitch (degrees, the module's convention) after an in-plane turn of the level picture by `turn` degrees."""
    from wildlifemapper_amd import attitude
    a = np.radians(turn)
    rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return attitude.attitude_rotation(roll, pitch) @ rz


def _explicit(name, size, out_size, rot, f_out=None, direct=False, **cam):
    c = camera(size, **cam)
    return dict(name=name, size=size, camera=c, rot=rot, out_size=out_size, keep=None, direct=direct,
                f_out=_spanning(size, out_size, c) if f_out is None else f_out)


def _kept(name, size, keep, rot, f_out=None, **cam):
    return dict(name=name, size=size, camera=camera(size, **cam), rot=rot, out_size=None, keep=keep, direct=False, f_out=f_out)


# Every source size of lens_cases and the quarter turn's 32 x 32, every output width and height, every kind of rotation at
# least once.  The explicit sizes take an f_out that spans the frame, so a tilted one has filled and sampled pixels; the kept
# ones take the default, f_out = fx.  direct: the case goes straight to the C entry, past rectify_plan, which would refuse it.
CASES = [
    _explicit("identity_five_33x129", (64, 129), (33, 129), IDENTITY, **FIVE),
    _explicit("identity_1x1", (5, 7), (1, 1), IDENTITY, f_out=0.83 * 7),
    _explicit("roll_pos_15x63", (5, 7), (15, 63), rotation(roll=8.0)),
    _explicit("roll_neg_16x64", (37, 53), (16, 64), rotation(roll=-6.0)),
    _explicit("pitch_pos_17x65", (37, 53), (17, 65), rotation(pitch=25.0), **BARREL),
    _explicit("pitch_neg_33x200", (130, 257), (33, 200), rotation(pitch=-5.0)),
    _explicit("both_five_33x65", (240, 320), (33, 65), rotation(roll=6.0, pitch=-4.0), f=260.0, **FIVE),
    _explicit("both_five_1x200", (240, 320), (1, 200), rotation(roll=-5.0, pitch=5.0), f=260.0, **FIVE),
    _explicit("both_five_33x1", (64, 129), (33, 1), rotation(roll=3.0, pitch=12.0), f_out=20.0, **FIVE),
    _explicit("turned_five_15x200", (64, 129), (15, 200), rotation(roll=4.0, pitch=3.0, turn=25.0), **FIVE),
    _explicit("fx_ne_fy_pp_off_17x129", (130, 257), (17, 129), rotation(roll=5.0, pitch=5.0), fy_over_fx=1.07, off=(7.25, -7.25), **FIVE),
    _explicit("quarter_turn_32x32", (32, 32), (32, 32), QUARTER, f=64.0, f_out=64.0, off=(0.0, 0.0)),
    _kept("valid_both_five", (240, 320), "valid", rotation(roll=6.0, pitch=-4.0), f=300.0, **FIVE),
    _kept("valid_pitch", (130, 257), "valid", rotation(pitch=5.0)),
    _kept("valid_roll_pp_off", (64, 129), "valid", rotation(roll=-4.0), off=(7.25, -7.25), **BARREL),
    _kept("all_both_five", (64, 129), "all", rotation(roll=-5.0, pitch=5.0), **FIVE),
    _kept("all_roll_barrel", (37, 53), "all", rotation(roll=8.0), **BARREL),
    # pitch 75 degrees and a level picture that looks 59 degrees either way (oh / (2 f_out) = 1.65): its upper rows look into the
    # frame, its middle rows past it, and its lower rows behind the camera (Z <= 0), the lowest of them with a (u, v) that lies
    # in the frame all the same -- the mirror image through the camera's centre, which only the Z > 0 test keeps out
    _explicit("z_both_signs_33x65", (240, 320), (33, 65), rotation(pitch=75.0), f=100.0, f_out=10.0, direct=True),
]
CASE_NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
WHOLE = ("identity_1x1", "quarter_turn_32x32")          # neither tilts: every pixel is sampled
Z_CASE = "z_both_signs_33x65"


def attitude_oracle(img, cam, rot, out_size, f_out, fill=FILL, modes=MODES, mutant=None):
    """The rule on a whole picture.  img (H,W,3) uint8, cam the nine numbers, rot (3,3) with d_cam = rot @ d_nadir, out_size
    (oh, ow).  Returns {'nearest', 'bilinear': (oh,ow,3) uint8, 'filled': the pixels that hold the fill colour, 'behind': those
    of them with Z <= 0, 'u', 'v': (oh,ow) float64, the rule's source positions}.  mutant: one of MUTANTS, a wrong rule."""
    h, w = img.shape[:2]
    oh, ow = out_size
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (F64(v) for v in cam)
    rot = np.asarray(rot, dtype=F64).reshape(3, 3)
    if mutant == "rot_transposed":
        rot = rot.T
    if mutant == "roll_flipped":
        rot = np.diag([-1.0, 1.0, 1.0]) @ rot @ np.diag([-1.0, 1.0, 1.0])        # the mirror image left-right: roll -> -roll
    if mutant == "pitch_flipped":
        rot = np.diag([1.0, -1.0, 1.0]) @ rot @ np.diag([1.0, -1.0, 1.0])        # the mirror image up-down: pitch -> -pitch
    r0, r1, r2_, r3, r4, r5, r6, r7, r8 = (F64(v) for v in rot.reshape(9))
    f_out = F64(f_out)

    def lens(x, y):
        r2 = x * x + y * y
        rad = F64(1.0) + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = x * rad + (((F64(2.0) * p1) * x) * y + p2 * (r2 + F64(2.0) * (x * x)))
        yd = y * rad + (p1 * (r2 + F64(2.0) * (y * y)) + ((F64(2.0) * p2) * x) * y)
        return xd, yd

    i = np.arange(ow, dtype=F64)[None, :]
    j = np.arange(oh, dtype=F64)[:, None]
    with np.errstate(all="ignore"):
        x = ((i + F64(0.5)) - F64(0.5) * F64(ow)) / f_out
        y = ((j + F64(0.5)) - F64(0.5) * F64(oh)) / f_out
        if mutant == "lens_before_rotation":
            x, y = lens(x, y)
        X = (r0 * x + r1 * y) + r2_
        Y = (r3 * x + r4 * y) + r5
        Z = (r6 * x + r7 * y) + r8
        if mutant == "r2_r5_dropped":
            X, Y = r0 * x + r1 * y, r3 * x + r4 * y
        front = Z > 0
        xn, yn = X / Z, Y / Z
        if mutant == "z_division_dropped":
            xn, yn = np.broadcast_arrays(X, Y)
        xd, yd = (xn, yn) if mutant == "lens_before_rotation" else lens(xn, yn)
        u = fx * xd + (cx + F64(0.5))
        v = fy * yd + (cy + F64(0.5))
        u, v, front = (np.broadcast_to(a, (oh, ow)) for a in (u, v, front))
        sees = inside(u, v, h, w) & (True if mutant == "z_test_dropped" else front)
    out = {"filled": int((~sees).sum()), "behind": int((~front).sum()), "u": u, "v": v}
    for m in modes:
        pic = np.empty((oh, ow, 3), dtype=np.uint8)
        pic[:] = np.asarray(fill, dtype=np.uint8)
        if sees.any():
            pic[sees] = _sample_many(img, u[sees], v[sees], m)
        out[m] = pic
    return out


def resolve(case):
    """The plan of a case (camera, size, out_size, f_out, rotation): through rectify_plan, the host layer under test, unless
    the case is direct."""
    from wildlifemapper_amd import attitude
    if case["direct"]:
        return {"camera": case["camera"], "size": case["size"], "out_size": case["out_size"], "f_out": case["f_out"], "rotation": case["rot"]}
    if case["keep"] is None:
        return attitude.rectify_plan(case["camera"], case["size"], case["rot"], out_size=case["out_size"], f_out=case["f_out"])
    return attitude.rectify_plan(case["camera"], case["size"], case["rot"], keep=case["keep"], f_out=case["f_out"])


def source_image(case):
    """The case's frame: noise, so that a position off by a fraction of a pixel changes bytes."""
    h, w = case["size"]
    return np.random.default_rng(2000 + CASE_NAMES.index(case["name"])).integers(0, 256, (h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(plan, frame, attitude_oracle's dict) of a case, computed once for all the tests that need it; treat as read-only."""
    case = BY_NAME[name]
    pl = resolve(case)
    img = source_image(case)
    return pl, img, attitude_oracle(img, pl["camera"], pl["rotation"], pl["out_size"], pl["f_out"])


# ---- a tilted camera over flat ground, in closed form ---------------------------------------------------------------------

def _to_level(yaw_deg):
    """Ground offsets (east, north) -> offsets (right, down) in the level picture, per metre: the inverse of nadir_affine's
    linear part over the ground sampling distance, which is its own inverse."""
    a = np.radians(yaw_deg)
    return np.array([[np.cos(a), -np.sin(a)], [-np.sin(a), -np.cos(a)]])


def forward_model(cam, rot, position, altitude, yaw_deg, ground):
    """Where the ground points (n,2) (east, north) appear in the RAW frame of a camera `altitude` above `position`: ground
    point -> ray of the level camera -> rot -> division -> lens.distort_points.  Test-owned, and no part of the rule's code."""
    from wildlifemapper_amd import lens
    d = (np.asarray(ground, dtype=F64) - np.asarray(position, dtype=F64)) @ _to_level(yaw_deg).T / altitude
    ray = np.concatenate([d, np.ones((len(d), 1))], axis=1) @ np.asarray(rot, dtype=F64).T          # d_cam = rot @ d_nadir
    pin = np.stack([cam[0] * (ray[:, 0] / ray[:, 2]) + (cam[2] + 0.5), cam[1] * (ray[:, 1] / ray[:, 2]) + (cam[3] + 0.5)], axis=1)
    return lens.distort_points(cam, pin)


def to_ground(georef, pts):
    """Pixel positions (n,2) -> ground points (n,2) under a nadir_affine georeference (2,3)."""
    return np.asarray(pts, dtype=F64) @ georef[:, :2].T + georef[:, 2]


CENSUS_RADIUS = 1.0


@functools.lru_cache(maxsize=None)
def census_scene():
    """Two 240 x 320 frames with f = 300 and the full lens, 30 m up and 8 m apart, banked opposite ways, and a dozen animals at
    least 3 m apart that both see.  Per frame: 'rot', 'position', 'yaw', 'raw' (12,2) the animals' raw positions by the
    forward model, 'plan' (keep='all'), 'raw_georef' what a caller without attitude would use, 'georef' the rectified one."""
    from wildlifemapper_amd import attitude, tiling
    size, alt = (240, 320), 30.0
    cam = camera(size, f=300.0, **FIVE)
    animals = np.array([(e, n) for n in (-6.0, 0.5, 6.0) for e in (-2.0, 2.5, 6.0, 10.0)]) + np.array([100.0, 200.0])
    frames = []
    for position, (roll, pitch), yaw in (((100.0, 200.0), (6.0, -4.0), 0.0), ((108.0, 200.0), (-5.0, 5.0), 3.0)):
        rot = attitude.attitude_rotation(roll, pitch)
        plan = attitude.rectify_plan(cam, size, rot, keep="all")
        oh, ow = plan["out_size"]
        frames.append(dict(rot=rot, position=position, yaw=yaw, plan=plan, raw=forward_model(cam, rot, position, alt, yaw, animals),
                           raw_georef=tiling.nadir_affine(*size, position, alt / cam[0], yaw),
                           georef=tiling.nadir_affine(oh, ow, position, alt / plan["f_out"], yaw)))
    return dict(size=size, camera=cam, altitude=alt, animals=animals, frames=frames)
