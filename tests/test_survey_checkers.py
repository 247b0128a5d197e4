"""The survey's checkers are themselves held in shape: the ground rule is restated in one file (tests/ground_oracle.py), its
shared geometry gives the values worked out by hand below, the analytic scene of the registration tests is written in one file
(tests/register_cases.py), and no test or tool imports a test module -- what two files share lives in a case or oracle module
(survey_util.py, ground_cases.py, ground_oracle.py, register_cases.py, pyramid_cases.py).  CPU only; the guards match patterns
in Python sources."""
import glob
import os
import re

import numpy as np

from ground_oracle import centre, inside, uv, window
from survey_util import ROOT

# the child-process scripts two GPU test files write out (each imports its own file), and one tool that drives the end-to-end test's engine
IMPORTS_OF_TEST_MODULES = {("tests/test_gpu_decoder.py", "test_gpu_decoder"), ("tests/test_gpu_ranges.py", "test_gpu_ranges"),
                           ("tools/fp8_tap_check.py", "test_gpu_e2e")}


def _sources(*folders):
    for folder in folders:
        for path in sorted(glob.glob(os.path.join(ROOT, folder, "*.py"))):
            with open(path) as f:
                yield folder + "/" + os.path.basename(path), f.read()


def test_no_module_imports_a_test_module():
    found = {(name, m.group(1)) for name, src in _sources("tests", "tools")
             for m in re.finditer(r"^\s*(?:from|import)\s+(test_\w+)", src, flags=re.M)}
    assert found == IMPORTS_OF_TEST_MODULES, sorted(found ^ IMPORTS_OF_TEST_MODULES)


def test_uv_expression_is_written_in_one_file():
    # (b0 * X + b1 * Y) + b2 with the coefficients indexed from any array, as every oracle used to spell it
    uv_expr = re.compile(r"\+\s*\w+\[[^\]]*1\]\s*\*\s*\w+\s*\)\s*\+\s*\w+\[[^\]]*2\]")
    assert [name for name, src in _sources("tests") if uv_expr.search(src)] == ["tests/ground_oracle.py"]


def test_analytic_scene_is_defined_in_one_file():
    # the ground of the refinement and pyramid tests and the frames' centres: a second copy would drift from the first
    for written in (r"^\s*def _scene_value\(", r"^\s*CENTRES\s*=\s*\(\("):
        assert [name for name, src in _sources("tests", "tools") if re.search(written, src, flags=re.M)] == ["tests/register_cases.py"], written


def test_shared_geometry_gives_the_hand_values():
    f64 = np.float64
    assert centre(f64(-0.25), f64(0.5), 0) == 0.0 and centre(f64(10.0), f64(0.7), 3) == f64(10.0) + f64(3.5) * f64(0.7)
    np.testing.assert_array_equal(centre(f64(1.0), f64(2.0), np.arange(3)), [2.0, 4.0, 6.0])
    assert type(centre(f64(0.0), f64(1.0), 2)) is np.float64
    # frame A of the hand cases: u = 2 X, v = 4 - 2 Y
    a = np.array([2.0, 0.0, 0.0, 0.0, -2.0, 4.0])
    assert uv(a, f64(3.0), f64(0.5)) == (6.0, 3.0)
    u, v = uv(np.stack([a, a + [0, 0, -4, 0, 0, 0]]), f64(3.0), f64(0.5))                  # every frame at once
    assert u.tolist() == [6.0, 2.0] and v.tolist() == [3.0, 3.0]
    u, v = uv(a, np.array([[0.0, 1.0, 4.0]]), np.array([[0.0], [2.0]]))                  # a window of cells
    assert u.tolist() == [[0.0, 2.0, 8.0]] * 2 and v.tolist() == [[4.0] * 3, [0.0] * 3]
    # the order of the sum: (b0 X + b1 Y) + b2, not b0 X + (b1 Y + b2) -- the second would lose the 1
    big = np.array([1e16, -1e16, 1.0, -1e16, 1e16, 1.0])
    assert uv(big, f64(1.0), f64(1.0)) == (1.0, 1.0)
    # half open: 0 is inside, w and h are not; a frame without pixels sees nothing
    assert inside(f64(0.0), f64(0.0), 4, 8) and inside(f64(7.999), f64(3.999), 4, 8)
    assert not inside(f64(8.0), f64(1.0), 4, 8) and not inside(f64(1.0), f64(4.0), 4, 8) and not inside(f64(-1e-300), f64(1.0), 4, 8)
    assert not inside(f64(0.0), f64(0.0), 0, 8) and not inside(f64(0.0), f64(0.0), 4, -3) and not inside(f64(np.nan), f64(0.0), 4, 8)
    # frame A's footprint [0, 4) x (0, 2] on cells of 1 m from (-10, -10): columns 10..13 and rows 10..11, two cells of margin
    assert window(a, 4, 8, f64(-10.0), f64(-10.0), f64(1.0), 30, 20) == (8, 16, 8, 14)
    assert window(a, 4, 8, f64(0.0), f64(0.0), f64(1.0), 5, 3) == (0, 5, 0, 3)               # clipped to the grid
    assert window(np.array([1.0, 2.0, 0.0, 2.0, 4.0, 0.0]), 4, 8, f64(0.0), f64(0.0), f64(1.0), 5, 3) == (0, 5, 0, 3)     # singular: the whole grid
    assert window(a, 0, 8, f64(0.0), f64(0.0), f64(1.0), 5, 3) is None and window(a + [np.nan, 0, 0, 0, 0, 0], 4, 8, 0.0, 0.0, 1.0, 5, 3) is None
