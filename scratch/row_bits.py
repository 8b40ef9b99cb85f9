"""SHA-256 of every output buffer, guard words included, that the row stages' GPU tests read back: the three SymbolMapper operations over
S.shapes() and S.MANY_ROWS on every constellation (tests/test_symbol_mapper_gpu.py), ConvolutionalCode.encode (and the decodes beside it) over
the shapes, rows and byte shifts of tests/test_conv_code_gpu.py, RateMatcher.match / unmatch / unmatch_hard over the calls of
tests/test_rate_match_gpu.py, the row above GFDM_HIP_RM_LDS_BITS among them.  The tests' own functions run (their assertions hold as well);
every Window.result() hashes the whole buffer first.  One line per test call: the number of its buffers and the SHA-256 over their digests
in the order they were read back.  One fresh process per library; two lists are equal line for line when two builds write the same bits.
    GFDM_HIP_LIB=<libgfdm_hip.so> python3 scratch/row_bits.py out_file                 -> profiles/r23/row_bits.txt"""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest                                         # the import paths of the suite
import gfdm_amd
import test_symbol_mapper_gpu as TS, test_conv_code_gpu as TC, test_rate_match_gpu as TR
import symbol_mapper_ref as S

lines, digests = [], []


def hashed(cls):
    inner = cls.result
    def result(self, *a):
        digests.append(hashlib.sha256(self.buf.cpu().numpy().tobytes()).hexdigest())
        return inner(self, *a)
    cls.result = result


def run(tag, fn, *a):
    del digests[:]
    fn(*a)
    lines.append("%-40s %4d buffers  %s" % (tag, len(digests), hashlib.sha256("".join(digests).encode()).hexdigest()))
    print(lines[-1], flush=True)


for mod in (TS, TC, TR):
    hashed(mod.Window)
gfdm_amd.set_jit(gfdm_amd.JIT_IN_CONSTRUCTOR)
mappers = {name: gfdm_amd.SymbolMapper(points) for name, (points, _) in S.constellations().items()}
for name in TS.NAMES:
    run("symbols every_shape %s" % name, TS.test_every_shape, name, mappers)
for name in S.MANY_ROWS_NAMES:
    run("symbols many_rows %s" % name, TS.test_many_rows, name, mappers)
for mode in TC.MODES:
    for n_info in TC.SHAPES:
        run("conv every_shape %s mode %s" % (n_info, mode), TC.test_every_shape, n_info, mode)
for n_rows, n_info in [(1, 3), (3, 3), (4, 3), (5, 3), (7, 3), (5000, 3), (32768 + 7, 2)]:
    run("conv rows_per_call %d x %d" % (n_rows, n_info), TC.test_rows_per_call, n_rows, n_info)
run("conv stride_and_alignment", TC.test_llr_stride_and_alignment, 0)
for count in (0, 3, 9, 10, 15, -2):
    run("conv count %d" % count, TC.test_count, count)
for n_coded in TR.SHAPES:
    run("rate every_shape %d" % n_coded, TR.test_every_shape, n_coded)
run("rate one_long_row", TR.test_one_long_row)
for n_rows, n_coded in [(1, 6), (3, 6), (4, 6), (5, 6), (7, 6), (5000, 6), (32768 + 7, 4)]:
    run("rate rows_per_call %d x %d" % (n_rows, n_coded), TR.test_rows_per_call, n_rows, n_coded)
for extra in (0, 1, 12):
    run("rate widths_and_alignment +%d" % extra, TR.test_widths_and_alignment, extra)
for count in (0, 3, 9, 10, 15, -2):
    run("rate count %d" % count, TR.test_count, count)
os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
open(sys.argv[1], "w").write("\n".join(lines) + "\n")
print("build %s: %d buffers in %d calls" % (gfdm_amd.build_id(), sum(int(l.split()[-3]) for l in lines), len(lines)))
