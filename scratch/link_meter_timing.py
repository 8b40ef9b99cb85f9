"""LinkMeter.measure (data-aided, all three outputs: both of its kernels) beside SymbolMapper.decode on the same symbols, for rocprofv3:
    rocprofv3 --kernel-trace --output-format csv -d out -o lm -- python3 scratch/link_meter_timing.py run
    python3 scratch/link_meter_timing.py summarise out/<host>/<pid>_kernel_trace.csv   -> profiles/r11/link_meter_kernel_durations.txt
The same run under rocprofv3 --pmc (counters only, eight at a time) gave profiles/r11/link_meter_counters.txt.
qam16 and gr_qpsk; 4096 rows of 468 symbols and 32768 rows of 5; WARM calls of each, then RUNS timed ones, decode and measure
alternating, the inputs rotating through a ring of four.  The summary drops the first WARM launches of every (kernel, grid) group."""
import csv
import os
import re
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("gr-gfdm_amd/python", "gr-gfdm_amd/lib")]

WARM, RUNS, RING = 3, 20, 4
SHAPES = ((4096, 468), (32768, 5))
NAMES = ("qam16", "gr_qpsk")


def points(name):
    import numpy as np
    if name == "gr_qpsk":
        return (np.array([-1 - 1j, 1 - 1j, -1 + 1j, 1 + 1j]) / np.sqrt(2)).astype(np.complex64)
    lv = np.array([-3, -1, 1, 3], np.float64)
    return ((lv[None, :] + 1j * lv[:, None]).ravel() / np.sqrt(10)).astype(np.complex64)


def run():
    import numpy as np
    import torch
    import gfdm_amd
    dev = torch.device("cuda:0")
    print("build %s  device %s  warm %d runs %d ring %d" % (gfdm_amd.build_id(), torch.cuda.get_device_name(0), WARM, RUNS, RING))
    for name in NAMES:
        p = points(name)
        mp, lm = gfdm_amd.SymbolMapper(p), gfdm_amd.LinkMeter(p)
        k = mp.bits_per_symbol()
        for n_rows, n_sym in SHAPES:
            rng = np.random.default_rng(n_rows)
            ring = []
            for _ in range(RING):
                data = torch.tensor(rng.integers(0, 256, (n_rows, mp.row_bytes(n_sym)), dtype=np.uint8), device=dev)
                x = mp.map(data, n_sym)
                x = x + 0.1 * torch.view_as_complex(torch.randn(n_rows, n_sym, 2, device=dev))
                ring.append((x.contiguous(), data))
            out_d = torch.empty(n_rows, mp.row_bytes(n_sym), dtype=torch.uint8, device=dev)
            outs = {"bit_errors": torch.empty(n_rows, dtype=torch.int32, device=dev), "err_power": torch.empty(n_rows, dtype=torch.float32, device=dev),
                    "ref_power": torch.empty(n_rows, dtype=torch.float32, device=dev)}
            ws = torch.empty(lm.measure_workspace_bytes(n_sym, n_rows), dtype=torch.uint8, device=dev)
            lm.reset()
            for i in range(WARM + RUNS):
                x, data = ring[i % RING]
                mp.decode(x, out=out_d)
                lm.measure(x, data, out=outs, workspace=ws)
            torch.cuda.synchronize()
            t = lm.totals()
            print("%s %dx%d k=%d: ber %.4f over %d bits" % (name, n_rows, n_sym, k, lm.ber(), t["bits"]))


def summarise(path):
    col = lambda r, *names: next(r[n] for n in names if n in r)
    groups = defaultdict(list)
    for r in csv.DictReader(open(path)):
        name = re.sub(r"\(.*$", "", col(r, "Kernel_Name").replace("(anonymous namespace)::", "").replace("void ", ""))
        if "k_symbols_decode" not in name and "k_meter_" not in name:
            continue
        grid = int(col(r, "Grid_Size_X", "Grid_Size")) // int(col(r, "Workgroup_Size_X", "Workgroup_Size"))
        groups[(name, grid)].append((int(col(r, "Start_Timestamp")), (int(col(r, "End_Timestamp")) - int(col(r, "Start_Timestamp"))) / 1e3))
    print("%-52s %10s %9s %10s %8s %8s" % ("kernel", "workgroups", "launches", "median_us", "min_us", "max_us"))
    for (name, grid), d in sorted(groups.items()):
        d = sorted(v for _, v in sorted(d)[WARM:])
        if d:
            print("%-52s %10d %9d %10.2f %8.2f %8.2f" % (name, grid, len(d), d[len(d) // 2], d[0], d[-1]))


if __name__ == "__main__":
    if sys.argv[1:2] == ["summarise"]:
        summarise(sys.argv[2])
    else:
        run()
