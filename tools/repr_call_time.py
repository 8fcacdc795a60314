#!/usr/bin/env python3
"""Time of the fused `utils.representation_grids` call alone at the C4 batch (6 x 65 x 480 x 640 -> normalised -> 384 x 512,
1 500 000 and 500 000 synthetic events per sample): median of 7 blocks of 20 calls after warm-up, three rotated input batches,
host clock ending in a device synchronise.  One line per process, tagged with the library it loaded -- for sweeps of a tuning
constant, one build each beside the product library (MPC_EXTRA_HIPCC_FLAGS=-DREPR_STRIP_KB=50 ... build_library(out=...), loaded
through MPC_AB_LIB), the product build first and last so that drift shows:
    python tools/repr_call_time.py; MPC_AB_LIB=build_ab/libmpcmax_s50.so python tools/repr_call_time.py; ...
The comparison inside one process is tools/repr_probe.py."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from motionpriorcmax_amd import build, utils  # noqa: E402
from oracle import repr_oracle as R  # noqa: E402

dev = torch.device('cuda:0')
B, CH, H, W, OUT = 6, 65, 480, 640, (384, 512)


def main():
    res = {}
    for n_ev in (1500000, 500000):
        batches = []
        for r in range(3):
            s = [R.synth_int_events(n_ev, (CH, H, W), 41234567, 41534567, 100 + 10 * r + b) for b in range(B)]
            x, y, p, t = (torch.stack([v[i] for v in s]).to(dev) for i in range(4))
            batches.append((x.float(), y.float(), p.float(), t))
        cnt = torch.full((B,), n_ev, dtype=torch.int32, device=dev)

        def call(i):
            x, y, p, t = batches[i % 3]
            return utils.representation_grids(x, y, p, t, cnt, CH, H, W, normalize=True, out_size=OUT, int_xy=True)

        for i in range(5):
            call(i)
        blocks = []
        for _ in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(20):
                call(i)
            torch.cuda.synchronize()
            blocks.append(1e3 * (time.perf_counter() - t0) / 20)
        res[n_ev] = round(statistics.median(blocks), 4)
    print(os.environ.get('MPC_AB_LIB', 'product build'), 'sources', build.source_hash(), 'median ms per call', res, flush=True)


if __name__ == '__main__':
    main()
