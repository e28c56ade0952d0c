"""Which forward Encoder::encode runs (csrc/fwd_mode.h forward_mode) and the profiler with profiling off (csrc/common.h
Profiler): host code only, no GPU.  Both are built into a small stand-alone program with AddressSanitizer and
UndefinedBehaviorSanitizer and the program asserts the table itself; nothing is loaded into python."""
import os
import subprocess

from lrp_imagecaptioning_amd.build import CSRC

MAIN = r"""
#include <cstdio>
#include <string>
#include <vector>
#include "common.h"
#include "fwd_mode.h"
using namespace lrp;
std::string& lrp::last_error_ref() { static std::string s; return s; }
static int bad = 0;
static void want(const char* what, bool bf16x3, bool fast, std::vector<int> cout, bool pool0, bool emit_ready, FwdMode mode, bool emit) {
  const FwdPlan p = forward_mode(bf16x3, fast, cout.data(), cout.size(), pool0, emit_ready);
  const bool ok = p.mode == mode && p.emit == emit;
  printf("%-28s mode %d emit %d %s\n", what, (int)p.mode, (int)p.emit, ok ? "ok" : "WRONG");
  if (!ok) ++bad;
}
int main() {
  const std::vector<int> vgg = {64, 64, 128, 128, 256};
  want("fp32", false, false, vgg, false, true, FWD_EXACT, false);
  want("bf16x3", true, false, vgg, false, true, FWD_PAIRS, true);
  want("bf16x3, LRP_FWD_EMIT=0", true, false, vgg, false, false, FWD_PAIRS, false);
  want("bf16x3_fast", true, true, vgg, false, true, FWD_FAST, false);
  want("a width of 12", true, false, {64, 12, 128}, false, true, FWD_EXACT, false);
  want("a width of 12, fast", true, true, {64, 12, 128}, false, true, FWD_EXACT, false);
  want("one layer", true, false, {64}, false, true, FWD_EXACT, false);
  want("one layer, fast", true, true, {64}, false, true, FWD_EXACT, false);
  want("layers[0].pool_after", true, false, vgg, true, true, FWD_PAIRS, false);
  want("layers[0].pool_after, fast", true, true, vgg, true, true, FWD_FAST, false);
  // profiling off: begin / end touch no event and book nothing; the entries report an empty list
  Profiler prof;
  for (int i = 0; i < 3; ++i) { prof.begin(nullptr); prof.end(nullptr, 1e9); }
  int64_t n = -1; double ms = -1, flop = -1, ms_out[4], flop_out[4]; int rows = -1;
  if (!prof.recs.empty() || prof.query(&n, &ms, &flop) != LRP_OK || n != 0 || ms != 0 || flop != 0) ++bad;
  if (prof.query(nullptr, nullptr, nullptr) != LRP_OK || prof.records(4, ms_out, flop_out, &rows) != LRP_OK || rows != 0) ++bad;
  printf("profiler off: %lld launches, %d rows\n", (long long)n, rows);
  return bad ? 1 : 0;
}
"""


def test_forward_mode_table_and_idle_profiler_under_sanitizers(tmp_path):
    src, exe = tmp_path / "fwd_mode_main.cpp", tmp_path / "fwd_mode_main"
    src.write_text(MAIN)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    hipcc = os.environ.get("HIPCC", os.path.join(rocm, "bin", "hipcc"))
    # host compile only (-x c++, sanitizers for the host alone): common.h needs the HIP runtime's declarations, the program
    # calls none of it and no device code is built
    flags = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc] + flags + ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
                                             "-o", str(exe), str(src), "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                                             "-Wl,-rpath," + os.path.join(rocm, "lib")])
    image = exe.read_bytes()
    assert b"__asan_init" in image and b"__ubsan_handle" in image     # the program really is instrumented
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert run.stdout.count(" ok\n") == 10 and "WRONG" not in run.stdout and "profiler off: 0 launches, 0 rows" in run.stdout
