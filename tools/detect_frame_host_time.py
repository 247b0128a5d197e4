"""Host-side cost of tiling.detect_frame alone: bench.py's N3 frame (6000 x 4000 resident, batch 16) with a stub model whose
records are canned, so the ~208 ms of the network are out of the picture: tile cut, merge and the Python around them.

  python tools/detect_frame_host_time.py [TREE]
      TREE: the checkout to import wildlifemapper_amd from (default: this one), so that two checkouts can be timed
      alternately.  5 warm-up calls, then 5 rounds of 40 calls, wall clock with a device synchronisation at both ends.
      Prints one JSON line.  No figure is a pass mark: the numbers are records (profiles/survey_python/).
"""
import json
import os
import sys
import time

import numpy as np
import torch

TREE = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TREE)
from wildlifemapper_amd import _native as N  # noqa: E402
from wildlifemapper_amd import tiling  # noqa: E402

dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
rec = torch.zeros((16, 51, 8), dtype=torch.float32)
c = rng.uniform(100, 900, (16, 51, 2))
rec[..., 0:2] = torch.from_numpy(c - 20).float()
rec[..., 2:4] = torch.from_numpy(c + 20).float()
rec[..., 4] = torch.from_numpy(rng.random((16, 51))).float()
ints = rec.view(torch.int32)
cand = rng.random((16, 51)) < 0.15
ints[..., 6] = torch.from_numpy(np.where(cand, N.FLAG_CONF | N.FLAG_SCORE | N.FLAG_NMS, N.FLAG_CONF).astype(np.int32))
rec = rec.to(dev)


class Stub:
    def detect(self, x, target_sizes=None):
        return {"records": rec[:x.shape[0]]}


frame = torch.randint(0, 256, (4000, 6000, 3), dtype=torch.uint8, device=dev)
m = Stub()
for _ in range(5):
    det = tiling.detect_frame(m, frame, batch=16)
torch.cuda.synchronize()
rounds = []
for _ in range(5):
    t0 = time.perf_counter()
    for _ in range(40):
        det = tiling.detect_frame(m, frame, batch=16)
    torch.cuda.synchronize()
    rounds.append(round((time.perf_counter() - t0) / 40 * 1e3, 4))
print(json.dumps({"tree": TREE, "ms_per_detect_frame_rounds": rounds, "min": min(rounds), "median": float(np.median(rounds)),
                  "detections": int(det["scores"].numel())}))
