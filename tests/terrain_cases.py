"""The survey terrain rule (include/wm_hip.h "Survey terrain") restated for the tests, the cases they share, the mutants that
show the cases have teeth, and the two-frame census scene over a hill.  The rule has no reference behaviour: terrain_oracle is
its restatement in numpy float64, written from the header statement for statement -- elementwise numpy arithmetic is one
correctly rounded IEEE operation per element and operator -- and the device must equal it byte for byte, with both counters.
The inside test and the sampling are the ground rules' (ground_oracle: inside, _sample_many), imported, not restated; cameras,
the fill and the modes are lens_cases'.

The host layer under test (wildlifemapper_amd.terrain) is used only to turn a position, a yaw and (roll, pitch) into a pose
and keep= into an output grid; every expected byte comes from terrain_oracle.  Pictures are at most about 100 x 150, frames
about 64 x 129 and DEMs 12 x 12 posts: the smallest shapes at which the kernel can still go wrong.  Nothing here asserts."""
import functools

import numpy as np

from ground_oracle import _sample_many, inside
from lens_cases import FILL, FIVE, MODES, camera  # noqa: F401

F64 = np.float64
POS = (512345.5, 9812345.25)              # UTM-sized: the order of the rule's subtractions shows at these magnitudes

MUTANTS = ("dem_south_up", "posts_at_corners", "du_sign", "m_transposed", "ia_wrapped", "weights_swapped", "z_test_dropped", "half_dropped")


def centred(heights, centre, cell):
    """(heights float32, (e0, n0), cell) of a DEM whose grid is centred on `centre`."""
    z = np.asarray(heights, dtype=np.float32)
    return z, (centre[0] - z.shape[1] * cell / 2, centre[1] + z.shape[0] * cell / 2), float(cell)


def post_positions(shape, origin, cell):
    """(E, N) of every post, (dh, dw) each: the cell centres of a north-up grid."""
    r, c = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    return origin[0] + (c + 0.5) * cell, origin[1] - (r + 0.5) * cell


def hill(shape, centre, cell, summit, height=25.0, sigma=20.0, base=100.0):
    """A Gaussian hill `height` high about `summit` on ground at `base`."""
    _, origin, _ = centred(np.zeros(shape), centre, cell)
    E, N = post_positions(shape, origin, cell)
    return centred(base + height * np.exp(-((E - summit[0]) ** 2 + (N - summit[1]) ** 2) / (2 * sigma ** 2)), centre, cell)


RAMP = dict(z0=100.0, sx=0.125, sy=-0.0625)              # z = z0 + sx (E - E_c) + sy (N - N_c): every post a float32 exactly


def ramp(shape, centre, cell, z0, sx, sy):
    _, origin, _ = centred(np.zeros(shape), centre, cell)
    E, N = post_positions(shape, origin, cell)
    return centred(z0 + sx * (E - centre[0]) + sy * (N - centre[1]), centre, cell)


def _case(name, size, dem, height, yaw, rot=None, position=POS, cam=None, direct=None, **plan):
    """A case: the frame's size, its camera, the DEM, the camera's height, yaw and (roll, pitch), and either ortho_plan's
    arguments (cell, yaw_deg, keep, out_size, centre) or direct = (out_size, georef), which goes past ortho_plan."""
    return dict(name=name, size=size, camera=camera(size, **(cam or {})), dem=dem, position=position, height=height, yaw=yaw, rot=rot,
                direct=direct, plan=plan)


def _hill_dem(shape=(12, 12)):
    return hill(shape, POS, 10.0, (POS[0] + 10.0, POS[1] + 5.0))


def _nodata_dem():
    z, o, c = _hill_dem()
    z = z.copy()
    z[3, 7], z[8, 4] = np.nan, np.inf
    return z, o, c


def _behind_dem():
    """Posts rising from 80 m in the west to 150 m in the east under a camera at 125 m: east of the 125 m contour Z <= 0."""
    return centred(np.tile(np.linspace(80.0, 150.0, 8), (8, 1)), POS, 10.0)


def _edge_dem():
    """4 x 4 posts a metre apart at the origin, a NaN where an unclamped ia would wrap to: flat index [0][4] is [1][0]."""
    z = np.array([[1.0, 2.0, 0.5, 1.5], [np.nan, 1.0, 2.5, 0.25], [0.75, 0.5, 1.0, 2.0], [1.25, 2.0, 0.5, 1.0]], dtype=np.float32)
    return z, (0.0, 4.0), 1.0


FLAT = centred(np.full((8, 8), 100.0), POS, 10.0)
HILL_KW = dict(height=160.0, yaw=30.0, rot=(4.0, 3.0), cam=FIVE)
# dem_edge: pixel centres at E = 0.25 + 0.5 (i + 0.5), so a = E - 0.5 is 3 = dem_w - 1 exactly at i = 6 and 3.5 at i = 7, and 0
# exactly at i = 0; N = 4.25 - 0.5 (j + 0.5), so b = 3.5 - N is 3 exactly at j = 7 and beyond at j = 8
EDGE_GEO = np.array([[0.5, 0.0, 0.25], [0.0, -0.5, 4.25]])

CASES = [
    _case("flat_identity", (33, 65), FLAT, 112.5, 0.0, cam=dict(f=50.0), cell=0.25, out_size=(33, 65)),
    _case("flat_yaw_0", (33, 65), FLAT, 112.5, 0.0, cam=dict(f=50.0), cell=0.25, yaw_deg=0.0, out_size=(33, 65)),
    _case("flat_yaw_90", (33, 65), FLAT, 112.5, 90.0, cam=dict(f=50.0), cell=0.25, yaw_deg=0.0, out_size=(65, 33)),
    _case("flat_yaw_180", (33, 65), FLAT, 112.5, 180.0, cam=dict(f=50.0), cell=0.25, yaw_deg=0.0, out_size=(33, 65)),
    _case("flat_yaw_270", (33, 65), FLAT, 112.5, 270.0, cam=dict(f=50.0), cell=0.25, yaw_deg=0.0, out_size=(65, 33)),
    _case("ramp", (64, 129), ramp((8, 8), POS, 10.0, **RAMP), 150.0, 20.0, cam=dict(f=100.0), cell=0.5, out_size=(70, 140)),
    _case("hill_five", (64, 129), _hill_dem(), keep="valid", **HILL_KW),
    _case("hill_five_all", (64, 129), _hill_dem(), keep="all", cell=0.6, **HILL_KW),
    _case("hill_north_up", (64, 129), _hill_dem(), keep="all", cell=0.75, yaw_deg=0.0, **HILL_KW),
    _case("hill_north_up_valid", (64, 129), _hill_dem(), keep="valid", yaw_deg=0.0, **HILL_KW),
    _case("off_dem", (37, 53), centred(np.linspace(99.0, 101.0, 16).reshape(4, 4), POS, 10.0), 130.0, 10.0, cam=dict(f=44.0), cell=0.5,
          out_size=(60, 100)),
    _case("nodata_post", (64, 129), _nodata_dem(), cell=0.6, out_size=(80, 130), **HILL_KW),
    _case("behind", (64, 129), _behind_dem(), 125.0, 0.0, cam=dict(f=30.0), cell=0.5, out_size=(33, 129)),
    _case("dem_edge", (37, 53), _edge_dem(), 12.0, 0.0, position=(2.0, 2.0), cam=dict(f=80.0), direct=((10, 9), EDGE_GEO)),
    _case("narrow_1x1", (64, 129), _hill_dem(), out_size=(1, 1), **HILL_KW),
    _case("narrow_1x63", (64, 129), _hill_dem(), out_size=(1, 63), **HILL_KW),
    _case("narrow_1x64", (64, 129), _hill_dem(), out_size=(1, 64), **HILL_KW),
    _case("narrow_17x65", (64, 129), _hill_dem(), out_size=(17, 65), cell=1.1, **HILL_KW),
    _case("narrow_33x1", (64, 129), _hill_dem(), out_size=(33, 1), cell=1.1, **HILL_KW),
    _case("one_row_dem_2x2", (37, 53), centred(np.array([[100.0, 104.0], [97.0, 109.0]]), POS, 30.0), 140.0, 200.0, rot=(-3.0, 2.0), cam=FIVE,
          cell=0.8, out_size=(50, 60)),
]
CASE_NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
YAW_CASES = {"flat_yaw_0": 0, "flat_yaw_90": -1, "flat_yaw_180": 2, "flat_yaw_270": 1}       # np.rot90's k of the nearest picture
VALID = [c["name"] for c in CASES if c["plan"].get("keep") == "valid" and "out_size" not in c["plan"]]
ALL = [c["name"] for c in CASES if c["plan"].get("keep") == "all"]


def terrain_oracle(img, cam, pose, dem, dem_geo, out_size, out_geo, fill=FILL, modes=MODES, mutant=None):
    """The rule on a whole picture.  img (H,W,3) uint8, cam the nine numbers, pose the twelve, dem (dh,dw) float32, dem_geo
    (e0, n0, dcell), out_size (oh, ow), out_geo the six numbers or a (2,3).  Returns {'nearest', 'bilinear': (oh,ow,3) uint8,
    'filled': the pixels that hold the fill colour, 'no_height': those of them without a height or with one that is not
    finite, 'behind': the pixels with a finite height and Z <= 0, 'u', 'v': (oh,ow) float64, the rule's source positions}.  mutant:
    one of MUTANTS, a deliberately wrong rule."""
    h, w = img.shape[:2]
    oh, ow = out_size
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (F64(v) for v in cam)
    pose = np.asarray(pose, dtype=F64).reshape(12)
    M = pose[3:].reshape(3, 3)
    if mutant == "m_transposed":
        M = M.T
    ce, cn, cu = (F64(v) for v in pose[:3])
    m0, m1, m2, m3, m4, m5, m6, m7, m8 = (F64(v) for v in M.reshape(9))
    dem = np.asarray(dem)
    assert dem.dtype == np.float32 and dem.ndim == 2
    if mutant == "dem_south_up":
        dem = dem[::-1]
    dem_h, dem_w = dem.shape
    flat = dem.reshape(-1)
    e0, n0, dcell = (F64(v) for v in dem_geo)
    g0, g1, g2, g3, g4, g5 = (F64(v) for v in np.asarray(out_geo, dtype=F64).reshape(6))
    half = F64(0.0) if mutant == "posts_at_corners" else F64(0.5)
    one = F64(1.0)
    px = np.arange(ow, dtype=F64)[None, :] + (F64(0.0) if mutant == "half_dropped" else F64(0.5))
    py = np.arange(oh, dtype=F64)[:, None] + (F64(0.0) if mutant == "half_dropped" else F64(0.5))
    with np.errstate(all="ignore"):
        E = (g0 * px + g1 * py) + g2
        N = (g3 * px + g4 * py) + g5
        a = (E - e0) / dcell - half
        b = (n0 - N) / dcell - half
        has = (0 <= a) & (a <= dem_w - 1) & (0 <= b) & (b <= dem_h - 1)
        fa, fb = np.floor(np.where(has, a, 0.0)).astype(np.int64), np.floor(np.where(has, b, 0.0)).astype(np.int64)
        ia, ib = (fa if mutant == "ia_wrapped" else np.minimum(fa, dem_w - 2)), np.minimum(fb, dem_h - 2)
        ta, tb = a - ia.astype(F64), b - ib.astype(F64)
        post = lambda r, c: flat[((ib + r) * dem_w + (ia + c)) % flat.size].astype(F64)      # in range unless ia is the mutant's
        z00, z01, z10, z11 = post(0, 0), post(0, 1), post(1, 0), post(1, 1)
        if mutant == "weights_swapped":
            z = (z00 * ta + z01 * (one - ta)) * (one - tb) + (z10 * ta + z11 * (one - ta)) * tb
        else:
            z = (z00 * (one - ta) + z01 * ta) * (one - tb) + (z10 * (one - ta) + z11 * ta) * tb
        dE, dN, dU = E - ce, N - cn, ((cu - z) if mutant == "du_sign" else (z - cu))
        X = (m0 * dE + m1 * dN) + m2 * dU
        Y = (m3 * dE + m4 * dN) + m5 * dU
        Z = (m6 * dE + m7 * dN) + m8 * dU
        front = has & (Z > 0)
        xn, yn = X / Z, Y / Z
        r2 = xn * xn + yn * yn
        rad = one + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = xn * rad + (((F64(2.0) * p1) * xn) * yn + p2 * (r2 + F64(2.0) * (xn * xn)))
        yd = yn * rad + (p1 * (r2 + F64(2.0) * (yn * yn)) + ((F64(2.0) * p2) * xn) * yn)
        u = fx * xd + (cx + F64(0.5))
        v = fy * yd + (cy + F64(0.5))
        sees = inside(u, v, h, w) & (has if mutant == "z_test_dropped" else front)
    out = {"filled": int((~sees).sum()), "no_height": int((~sees & ~(has & np.isfinite(z))).sum()), "behind": int((has & np.isfinite(z) & ~(Z > 0)).sum()),
           "u": u, "v": v, "sees": sees}
    for m in modes:
        pic = np.empty((oh, ow, 3), dtype=np.uint8)
        pic[:] = np.asarray(fill, dtype=np.uint8)
        if sees.any():
            pic[sees] = _sample_many(img, u[sees], v[sees], m)
        out[m] = pic
    return out


def resolve(case):
    """(dem, plan) of a case: the terrain_grid, and ortho_plan's dict -- through ortho_plan, the host layer under test, unless
    the case is direct."""
    from wildlifemapper_amd import terrain
    dem = terrain.terrain_grid(*case["dem"])
    pose = terrain.camera_pose(case["position"], case["height"], case["yaw"], case["rot"])
    if case["direct"] is None:
        return dem, terrain.ortho_plan(case["camera"], case["size"], pose, dem, **case["plan"])
    out_size, georef = case["direct"]
    return dem, {"camera": case["camera"], "size": case["size"], "out_size": out_size, "pose": pose, "georef": np.asarray(georef, dtype=F64),
                 "cell": None, "yaw_deg": None, "dem_origin": dem["origin"], "dem_cell": dem["cell"], "dem_size": dem["heights"].shape}


def dem_geo(dem):
    return (*dem["origin"], dem["cell"])


def source_image(case):
    """The case's frame: noise, so that a position off by a fraction of a pixel changes bytes."""
    h, w = case["size"]
    return np.random.default_rng(3000 + CASE_NAMES.index(case["name"])).integers(0, 256, (h, w, 3), dtype=np.uint8)


def oracle_of(pl, dem, img, **kw):
    return terrain_oracle(img, pl["camera"], pl["pose"], dem["heights"], dem_geo(dem), pl["out_size"], pl["georef"], **kw)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(plan, dem, frame, terrain_oracle's dict) of a case, computed once for all the tests that need it; treat as read-only."""
    case = BY_NAME[name]
    dem, pl = resolve(case)
    img = source_image(case)
    return pl, dem, img, oracle_of(pl, dem, img)


# ---- two frames over a hill: the census that is wrong on a flat georeference -------------------------------------------------

CENSUS_RADIUS = 1.0


@functools.lru_cache(maxsize=None)
def census_scene():
    """Two level 120 x 160 frames with f = 150 and no lens model (the error shown is the relief's alone), 120 m above ground at 0 m on which a hill 25 m high stands,
    their nadir points 30 m either side of the summit, and twelve animals on the slopes at least 3 m apart.  'dem', 'camera',
    'size', 'animals' (12,2) ground positions; per frame 'pose', 'position', 'yaw', 'plan' (keep='valid'), 'raw' (12,2) the
    animals' raw positions by the rule (terrain_points(to='raw')), 'flat_georef' what a caller without a DEM would use: the
    plane at 0 m."""
    from wildlifemapper_amd import terrain, tiling
    size, alt, summit = (120, 160), 120.0, (100.0, 200.0)
    cam = camera(size, f=150.0)
    dem = terrain.terrain_grid(*hill((11, 11), summit, 20.0, summit, height=25.0, sigma=25.0, base=0.0))      # a post on the summit
    animals = np.array([(e, n) for n in (-14.0, 1.5, 15.0) for e in (-21.0, -8.0, 7.0, 20.0)]) + np.array(summit)
    frames = []
    for position, yaw in (((70.0, 200.0), 0.0), ((130.0, 203.0), 5.0)):
        pose = terrain.camera_pose(position, alt, yaw)
        plan = terrain.ortho_plan(cam, size, pose, dem, keep="valid")
        frames.append(dict(pose=pose, position=position, yaw=yaw, plan=plan, raw=terrain.terrain_points(plan, dem, animals, to="raw"),
                           flat_georef=tiling.nadir_affine(*size, position, alt / cam[0], yaw)))
    return dict(size=size, camera=cam, altitude=alt, dem=dem, animals=animals, frames=frames)


def to_ground(georef, pts):
    """Pixel positions (n,2) -> ground points (n,2) under a (2,3) georeference."""
    return np.asarray(pts, dtype=F64) @ georef[:, :2].T + georef[:, 2]


# ---- the attitude kernel as an independent check: a flat DEM under a rectified picture's own grid ---------------------------

TWINS = ("valid_both_five", "valid_pitch", "valid_roll_pp_off")          # the attitude cases that fill nothing
TWIN_YAW, TWIN_ALTITUDE, TWIN_GROUND = 25.0, 30.0, 100.0


@functools.lru_cache(maxsize=None)
def rectify_twin(name):
    """An attitude case as a terrain case: its camera `TWIN_ALTITUDE` above a flat DEM, the output grid the rectified picture's
    own georeference, nadir_affine(oh, ow, position, altitude / f_out, yaw).  Returns (attitude plan, frame, ortho plan, dem,
    differs): differs (oh, ow) bool marks the pixels at which the two rules' source positions -- terrain_oracle's (u, v) and
    attitude_points(to='raw') -- fall into different frame pixels; they round differently, and only there may the nearest
    pictures of wm_ortho_u8 and wm_rectify_u8 differ."""
    import attitude_cases as AC
    from wildlifemapper_amd import attitude, terrain, tiling
    apl, img, _ = AC.expected(name)
    oh, ow = apl["out_size"]
    dem = terrain.terrain_grid(*centred(np.full((8, 8), TWIN_GROUND), POS, 10.0))
    pose = terrain.camera_pose(POS, TWIN_GROUND + TWIN_ALTITUDE, TWIN_YAW, apl["rotation"])
    georef = tiling.nadir_affine(oh, ow, POS, TWIN_ALTITUDE / apl["f_out"], TWIN_YAW)
    pl = {"camera": apl["camera"], "size": apl["size"], "out_size": (oh, ow), "pose": pose, "georef": georef, "cell": TWIN_ALTITUDE / apl["f_out"],
          "yaw_deg": TWIN_YAW, "dem_origin": dem["origin"], "dem_cell": dem["cell"], "dem_size": dem["heights"].shape}
    want = oracle_of(pl, dem, img, modes=())
    jj, ii = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
    uv = attitude.attitude_points(apl, np.stack([ii.ravel() + 0.5, jj.ravel() + 0.5], axis=1), to="raw")
    differs = (np.floor(uv[:, 0]).reshape(oh, ow) != np.floor(want["u"])) | (np.floor(uv[:, 1]).reshape(oh, ow) != np.floor(want["v"]))
    return apl, img, pl, dem, differs | ~want["sees"]
