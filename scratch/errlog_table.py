"""Worst measured error per path from a GFDM_ERRLOG file (tests/conftest.py::check_err): python scratch/errlog_table.py <errlog>
With --taps: the taps_<route>_<family>_<entry> lines of tests/test_taps_gpu.py, worst per route and tap family.
With --accuracy: the acc_<route>_<taps>_<entry>_<figure> lines of tests/test_accuracy_gpu.py: per tag the measured figure, its bound, and the
ratio of both to the figure of the plain-C float32 oracle on the same call (the accref_... line in front of each) and the margin
of the bound (the accmargin_... line)."""
import collections, re, sys
worst = collections.defaultdict(lambda: (0.0, 0.0, 0))
if "--accuracy" in sys.argv:
    sys.argv.remove("--accuracy")
    ref, margin, rows, cross = {}, {}, [], []
    for line in open(sys.argv[1]):
        tag, err, tol = line.split()
        if tag.startswith("accref_"):
            ref[tag[len("accref_"):]] = float(err)
        elif tag.startswith("accmargin_"):
            margin[tag[len("accmargin_"):]] = float(err)
        elif tag.endswith("_mx_vs_valu"):
            cross.append((tag, float(err), float(tol)))
        elif tag.startswith("acc_"):
            rows.append((tag, float(err), float(tol), ref[tag[len("acc_"):]], margin[tag[len("acc_"):]]))
    worst = max(rows, key=lambda r: r[1] / r[3])
    print("Measured figure of the HIP path, its bound, and both as multiples of the plain-C float32 oracle's figure on the same call")
    print("(`GFDM_ERRLOG=<file> pytest tests/test_accuracy_gpu.py -m gpu`, `scratch/errlog_table.py --accuracy <file>`).")
    print("%d comparisons; worst measured ratio %.2f (`%s`).\n" % (len(rows), worst[1] / worst[3], worst[0]))
    print("| figure | margin (bound / reference) | measured / reference: least | median | largest |\n|---|---|---|---|---|")
    for fig in ("l2", "peak", "pos"):
        r = sorted(x[1] / x[3] for x in rows if x[0].endswith("_" + fig))
        m = sorted({x[4] for x in rows if x[0].endswith("_" + fig)})
        print("| `%s` | %s | %.2f | %.2f | %.2f |" % (fig, ", ".join("%g" % v for v in m), r[0], r[len(r) // 2], r[-1]))
    if cross:
        print("\nThe matrix-core cancellation rounds against the vector-ALU rounds on the same call (bits differ, asserted):\n\n| tag | relative L2 | bound |\n|---|---|---|")
        for tag, err, tol in cross:
            print("| `%s` | %.2e | %.0e |" % (tag, err, tol))
    print("\nThe bound is the margin times the reference figure (the log keeps two digits of it).\n")
    print("| tag | measured | bound | reference | measured / reference | margin |\n|---|---|---|---|---|---|")
    for tag, err, tol, rf, mg in rows:
        print("| `%s` | %.2e | %.1e | %.2e | %.2f | %g |" % (tag, err, tol, rf, err / rf, mg))
    sys.exit(0)
if "--taps" in sys.argv:
    sys.argv.remove("--taps")
    fams = ("rand", "real_asym", "cplx_icsym")
    cell, other = collections.defaultdict(lambda: (0.0, "", 0)), collections.defaultdict(lambda: (0.0, 0.0, 0))
    for line in open(sys.argv[1]):
        tag, err, tol = line.split()
        m = re.match(r"taps_(\w+?)_(%s)_(\w+)$" % "|".join(fams), tag)
        if "taps_" not in tag:
            continue
        if m and float(tol) == 1e-5 and "_cross_" not in tag and not m.group(1).startswith(("tx_", "pybind_")) and not m.group(3).startswith("frames") and m.group(3) != "dem":
            w, e, n = cell[m.group(1), m.group(2)]
            cell[m.group(1), m.group(2)] = (max(w, float(err)), m.group(3) if float(err) > w else e, n + 1)
        else:                                    # everything else, the route, family and input taken out of the tag
            key = re.sub(r"rxl_ctaps_\w+_(qpsk|gauss)$", "fixtures", tag)
            key = re.sub(r"^taps_(rowlane|generic|rader)_(jit_)?[a-z0-9]+?(_per_wave|_12|_dft)?_(%s|imag|above|frames)" % "|".join(fams), r"taps_<route>_\4", key)
            key = re.sub(r"_(mf|zf|ts|sc)(_|$)", r"\2", re.sub(r"_(generic|rowlane)_rand", "_<family>_rand", re.sub(r"framed\d", "framed", key)))
            key = re.sub(r"taps_(rowlane_7|rowlane_jit|generic_5_32)_rand_dem", "taps_<burst case>_rand_dem", key)
            w, t, n = other[key]
            other[key] = (max(w, float(err)), max(t, float(tol)), n + 1)
    print("| route | comparisons per family | " + " | ".join("`%s`: worst error (entry point)" % f for f in fams) + " |\n|---|---|" + "---|" * len(fams))
    for route in sorted({r for r, _ in cell}):
        print("| `%s` | %d | " % (route, cell[route, fams[0]][2]) + " | ".join("%.2e (%s)" % cell[route, f][:2] for f in fams) + " |")
    print("\n| other comparison | count | worst error | bound |\n|---|---|---|---|")
    for key, (w, t, n) in sorted(other.items()):
        print("| `%s` | %d | %.2e | %.0e |" % (key, n, w, t))
    sys.exit(0)
for line in open(sys.argv[1]):
    tag, err, tol = line.split()
    fam = re.sub(r"_(\d+_\d+_\d+.*|ic_.*|ref_.*|cfg.*|rxl_.*)$", "", tag)
    fam = re.sub(r"_\d+_\d+$", "", fam)
    fam = {"golden_ic_mf": "MF + IC vs pygfdm rounds", "golden_ic_zf": "ZF + IC vs pygfdm rounds", "golden": "MF / ZF + IC vs the pygfdm IC rounds",
           "golden_rx_overlap": "receiver at overlap 2 .. 8 vs pygfdm gfdm_demodulate_fft_loop", "golden_rx_overlap_S": "fft_filter_downsample at overlap 2 .. 8 vs the same model"}.get(fam, fam)
    w, t, n = worst[fam]
    worst[fam] = (max(w, float(err)), float(tol), n + 1)
print("| path | comparisons | worst relative error | bound |\n|---|---|---|---|")
for fam, (w, t, n) in sorted(worst.items()):
    print("| %s | %d | %.2e | %.0e |" % (fam, n, w, t))
