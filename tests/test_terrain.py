"""Survey terrain on the GPU: wm_ortho_u8 equals the rule's restatement (tests/terrain_cases.py: terrain_oracle) byte for byte,
with both counters, for every case in both modes at every byte offset of the output; over flat ground, with the output grid
set to a rectified picture's own georeference, it equals wm_rectify_u8's output everywhere the two rules' source positions
fall into the same frame pixel; and preprocess.ortho_u8 and tiling.orthorectified hand those bytes to mosaic unchanged.  The
census at the end is wrong on a flat georeference and exact over the DEM.  The cases, the oracle, the mutants and the CPU proofs
that the twins and the census scene are what they claim are in tests/terrain_cases.py and tests/test_terrain_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import attitude_cases as AC
import terrain_cases as TC
from survey_util import DEV, _guarded, _Lazy, _lib, _up
from wildlifemapper_amd import _native as N
from wildlifemapper_amd import preprocess, terrain, tiling

pytestmark = pytest.mark.gpu
MODE = {"nearest": N.MOSAIC_NEAREST, "bilinear": N.MOSAIC_BILINEAR}


def _args(pl, dem):
    """The host-side arrays of a plan and its DEM as wm_ortho_u8 takes them: (camera, pose, dem_geo, out_geo)."""
    return ((C.c_double * 9)(*np.asarray(pl["camera"]).tolist()), (C.c_double * 12)(*np.asarray(pl["pose"]).tolist()),
            (C.c_double * 3)(*TC.dem_geo(dem)), (C.c_double * 6)(*np.asarray(pl["georef"]).reshape(6).tolist()))


def _ortho_at(pl, dem, img, mode, out_off, in_off, fill=TC.FILL, out_buf=None):
    """wm_ortho_u8 with the input in_off and the output out_off bytes past an aligned allocation, both inside guard bytes
    (survey_util._guarded: 255 all round), the DEM and the two counters in guarded allocations too.  Returns (picture, filled,
    no_height, the output's whole buffer)."""
    lib = _lib()
    (h, w), (oh, ow) = pl["size"], pl["out_size"]
    dh, dw = dem["heights"].shape
    _, src = _guarded(img, in_off, DEV)
    _, posts = _guarded(dem["heights"], 8, DEV)
    if out_buf is None:
        out_buf = _guarded(np.full((oh, ow, 3), 171, np.uint8), out_off, DEV)[0]
    stats_buf, stats = _guarded(np.full(2, -5, np.int64), 16, DEV)
    cam, pose, dgeo, ogeo = _args(pl, dem)
    N.check(lib.wm_ortho_u8(C.c_void_p(src.data_ptr()), h, w, cam, pose, C.c_void_p(posts.data_ptr()), dh, dw, dgeo, C.c_void_p(out_buf.data_ptr() + out_off),
                            oh, ow, ogeo, MODE[mode], (C.c_uint8 * 3)(*fill), C.c_void_p(stats.data_ptr()), N.stream_ptr(torch.device(DEV))))
    got = out_buf.cpu().numpy()
    n = oh * ow * 3
    assert (got[:out_off] == 255).all() and (got[out_off + n:] == 255).all(), "the kernel wrote outside its output"
    s = stats_buf.cpu().numpy()
    assert (s[:16] == 255).all() and (s[32:] == 255).all(), "the kernel wrote outside its two counters"
    filled, no_height = (int(v) for v in s[16:32].view(np.int64))
    return got[out_off:out_off + n].reshape(oh, ow, 3), filled, no_height, out_buf


@pytest.mark.parametrize("name", TC.CASE_NAMES)
def test_ortho_equals_the_oracle_byte_for_byte(name):
    pl, dem, img, want = TC.expected(name)
    for mode in TC.MODES:
        for off in range(4):                                              # the output 0..3 bytes past a dword; the input at another offset
            got, filled, no_height, _ = _ortho_at(pl, dem, img, mode, off, (off + 1) % 4)
            diff = int((got != want[mode]).sum())
            assert diff == 0, (name, mode, off, diff, np.argwhere((got != want[mode]).any(axis=2))[:4].tolist())
            assert (filled, no_height) == (want["filled"], want["no_height"]), (name, mode, off)


def _rectify(apl, img, mode):
    """wm_rectify_u8 on an attitude plan: the existing kernel."""
    out = torch.empty((*apl["out_size"], 3), dtype=torch.uint8, device=DEV)
    src = torch.from_numpy(img).to(DEV)
    N.check(_lib().wm_rectify_u8(N.ptr(src), *apl["size"], (C.c_double * 9)(*apl["camera"].tolist()), (C.c_double * 9)(*apl["rotation"].reshape(9).tolist()),
                                 N.ptr(out), *apl["out_size"], apl["f_out"], MODE[mode], (C.c_uint8 * 3)(*TC.FILL), None, N.stream_ptr(torch.device(DEV))))
    return out.cpu().numpy()


@pytest.mark.parametrize("name", TC.TWINS)
def test_flat_ground_equals_rectify_where_the_two_rules_sample_the_same_pixel(name):
    """The existing kernel as an independent check: over a flat DEM, the output grid the rectified picture's own georeference,
    the nearest orthophoto equals wm_rectify_u8's nearest picture everywhere but on the set, computed on the CPU from the two
    host restatements and held there to at most 0.1 % of the picture, where the two rules' source positions fall into different
    frame pixels."""
    apl, img, pl, dem, differs = TC.rectify_twin(name)
    assert differs.mean() <= 1e-3
    got, filled, no_height, _ = _ortho_at(pl, dem, img, "nearest", 0, 0)
    want = _rectify(apl, img, "nearest")
    same = (got == want).all(axis=2)
    assert (filled, no_height) == (0, 0) and (same | differs).all(), (name, int((~same).sum()), int(differs.sum()))


def test_quarter_turns_through_the_kernel_are_rot90():
    for name, k in TC.YAW_CASES.items():
        pl, dem, img, _ = TC.expected(name)
        got, filled, no_height, _ = _ortho_at(pl, dem, img, "nearest", 0, 0)
        assert np.array_equal(got, np.rot90(img, k)) and (filled, no_height) == (0, 0), name


def test_a_second_call_overwrites_every_byte():
    for name in ("hill_north_up", "nodata_post", "behind"):
        pl, dem, img, want = TC.expected(name)
        for mode in TC.MODES:
            _, _, _, buf = _ortho_at(pl, dem, img, mode, 1, 0, fill=(200, 100, 50))
            got, filled, no_height, _ = _ortho_at(pl, dem, img, mode, 1, 0, out_buf=buf)
            assert np.array_equal(got, want[mode]) and (filled, no_height) == (want["filled"], want["no_height"]), (name, mode)


def test_no_stats_pointer_is_accepted():
    pl, dem, img, want = TC.expected("off_dem")
    out = torch.empty((*pl["out_size"], 3), dtype=torch.uint8, device=DEV)
    src, posts = torch.from_numpy(img).to(DEV), torch.from_numpy(dem["heights"]).to(DEV)
    cam, pose, dgeo, ogeo = _args(pl, dem)
    N.check(_lib().wm_ortho_u8(N.ptr(src), *pl["size"], cam, pose, N.ptr(posts), *dem["heights"].shape, dgeo, N.ptr(out), *pl["out_size"], ogeo,
                               N.MOSAIC_BILINEAR, (C.c_uint8 * 3)(*TC.FILL), None, N.stream_ptr(torch.device(DEV))))
    assert np.array_equal(out.cpu().numpy(), want["bilinear"])


NEAR = ((0.0, 0.0, 160.0, 30.0, (4.0, 3.0)), (2.0, -1.0, 157.0, 33.0, (-2.0, 2.0)), (-1.0, 2.0, 155.0, 27.0, (0.0, -3.0)))      # every border ray meets the DEM
APART = ((0.0, 0.0, 160.0, 30.0, (4.0, 3.0)), (9.0, -4.0, 163.0, 35.0, (-5.0, 5.0)), (-7.0, 6.0, 158.0, 21.0, (0.0, -6.0)))


def _per_frame(where=NEAR):
    """Three frames of one camera and size over the hill, each with its own pose (east and north of terrain_cases.POS, height,
    yaw, (roll, pitch)): (camera, size, dem, poses (3,12), frames)."""
    case = TC.BY_NAME["hill_five"]
    size, cam = case["size"], case["camera"]
    dem = terrain.terrain_grid(*case["dem"])
    poses = np.stack([terrain.camera_pose((TC.POS[0] + e, TC.POS[1] + n), height, yaw, rot) for e, n, height, yaw, rot in where])
    rng = np.random.default_rng(12)
    frames = [rng.integers(0, 256, (*size, 3), dtype=np.uint8) for _ in poses]
    return cam, size, dem, poses, frames


def test_wrappers_return_the_oracles_bytes():
    """preprocess.ortho_u8 and tiling.orthorectified, device and host frames, a plan and a size per frame; the DEM goes up once;
    a lazy source is indexed once per access."""
    _lib()
    pl, dem, img, want = TC.expected("nodata_post")
    dem = terrain.terrain_grid(dem["heights"], dem["origin"], dem["cell"])          # a dict of this test's own: to_device() writes into it
    dev_frame = torch.from_numpy(img).to(DEV)
    assert dem["device_heights"] is None
    for mode in TC.MODES:
        got, counts = preprocess.ortho_u8(dev_frame, pl, dem, sample=mode, fill=TC.FILL, count=True)
        assert got.shape == (*pl["out_size"], 3) and got.dtype == torch.uint8 and got.device == dev_frame.device
        assert counts.dtype == torch.int64 and counts.is_cuda and counts.tolist() == [want["filled"], want["no_height"]]
        assert np.array_equal(got.cpu().numpy(), want[mode]), mode
    posts = dem["device_heights"]
    assert posts.is_cuda and posts.dtype == torch.float32 and np.array_equal(posts.cpu().numpy(), dem["heights"], equal_nan=True)
    assert np.array_equal(preprocess.ortho_u8(dev_frame, pl, dem, fill=TC.FILL).cpu().numpy(), want["bilinear"])
    assert dem["device_heights"] is posts                                   # uploaded once
    given = terrain.terrain_grid(posts, dem["origin"], dem["cell"])         # a device tensor is kept as it is
    assert given["device_heights"].data_ptr() == posts.data_ptr() and np.array_equal(given["heights"], dem["heights"], equal_nan=True)
    assert terrain.terrain_grid(dem["heights"], dem["origin"], dem["cell"], device=DEV)["device_heights"].is_cuda
    with pytest.raises(ValueError, match="the plan was made for"):
        preprocess.ortho_u8(dev_frame[:-1], pl, dem)
    cam, size, dem, poses, frames = _per_frame()
    src = _Lazy([torch.from_numpy(frames[0]).to(DEV), frames[1], torch.from_numpy(frames[2])])       # a device tensor, a numpy array, a CPU tensor
    o = tiling.orthorectified(src, cam, poses, dem, keep="all", cell=0.6, sample="nearest", fill=TC.FILL, size=size)
    assert len(o) == 3 and src.asked == [] and o.sizes.shape == (3, 2) and len({tuple(s) for s in o.sizes}) == 3 and o.georef.shape == (3, 2, 3)
    wants = [TC.oracle_of(p, dem, f, modes=("nearest",))["nearest"] for f, p in zip(frames, o.plans)]
    for i in (2, 0, 1):
        got = o[i]
        assert got.is_cuda and tuple(got.shape[:2]) == tuple(o.sizes[i]) and np.array_equal(got.cpu().numpy(), wants[i]), i
    assert src.asked == [2, 0, 1]
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(o, wants)) and src.asked == [2, 0, 1, 0, 1, 2]
    with pytest.raises(ValueError, match="the plan was made for"):
        tiling.orthorectified([frames[0][:, :-1]], cam, poses[:1], dem, size=size)[0]


def test_mosaic_of_orthophotos_equals_mosaic_of_the_oracles_pictures():
    _lib()
    cam, size, dem, poses, frames = _per_frame(APART)
    src = _Lazy(frames)
    o = tiling.orthorectified(src, cam, poses, dem, keep="valid", sample="bilinear", size=size)
    got = tiling.mosaic(o, o.georef, 0.4, sizes=o.sizes)
    pictures = [TC.oracle_of(p, dem, f, fill=(0, 0, 0), modes=("bilinear",))["bilinear"] for f, p in zip(frames, o.plans)]
    want = tiling.mosaic(pictures, o.georef, 0.4)
    assert torch.equal(got["mosaic"], want["mosaic"]) and torch.equal(got["source"], want["source"])
    assert sorted(src.asked) == torch.nonzero(want["won"] > 0).flatten().tolist() and len(src.asked) >= 2       # the winners, once each


def _census_results(centres):
    """One detect_frames-like result per frame: a 6 x 6 box about each centre (n,2)."""
    out = []
    for c in centres:
        boxes = np.concatenate([c - 3.0, c + 3.0], axis=1).astype(np.float32)
        out.append({"boxes": _up(boxes), "scores": _up(np.linspace(0.9, 0.5, len(c)).astype(np.float32)),
                    "labels": torch.ones(len(c), device=DEV, dtype=torch.int64)})
    return out


def test_census_counts_each_animal_once_only_over_the_dem():
    """Two level frames either side of a 25 m hill over a dozen animals on its slopes (terrain_cases.census_scene, proved on the
    CPU: every flat position is off by more than the radius, no two of different frames within it; over the DEM each is within
    1e-6 m of its animal).  With the flat nadir_affine on the raw centres the census finds more individuals than animals; with
    the centres through terrain_points(to='ground') and an identity georeference it finds exactly the animals, two members
    each; and so it does with boxes placed in the orthophotos, through to='picture' and the sequence's own georef.  Without the
    feature there is no terrain_points, and only the first count exists."""
    _lib()
    sc = TC.census_scene()
    n, dem, frames = len(sc["animals"]), sc["dem"], sc["frames"]
    flat = tiling.census(_census_results([f["raw"] for f in frames]), np.stack([f["flat_georef"] for f in frames]), radius=TC.CENSUS_RADIUS)
    assert flat["count"] > n, flat["count"]

    def exact(result):
        assert result["count"] == n == 12 and result["members"].tolist() == [2] * n
        who = [int(v) for v in result["individual"]]                       # detections in frame order: animal k is k and n + k
        assert who[:n] == who[n:] and len(set(who[:n])) == n

    ground = [tiling.terrain_points(f["plan"], dem, f["raw"], to="ground") for f in frames]
    identity = np.tile(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (2, 1, 1))
    exact(tiling.census(_census_results(ground), identity, radius=TC.CENSUS_RADIUS))
    o = tiling.orthorectified([np.zeros((*sc["size"], 3), np.uint8)] * 2, sc["camera"], np.stack([f["pose"] for f in frames]), dem, size=sc["size"])
    assert all(np.array_equal(g, f["plan"]["georef"]) for g, f in zip(o.georef, frames))
    exact(tiling.census(_census_results([tiling.terrain_points(p, dem, g, to="picture") for p, g in zip(o.plans, ground)]), o.georef,
                        radius=TC.CENSUS_RADIUS))
