"""The graph kernel headers of dsk_amd/csrc can meet in one translation unit: a source file that includes all twelve of them (query.h,
graph.h, unitigs.h, rules.h, rowfilter.h, tips.h, bubbles.h, connections.h, variants.h, thread.h, components.h, correct.h) passes the
compiler's syntax check for gfx950 with the flags of dsk_amd/csrc/Makefile.  Before rules.h and rowfilter.h existed, the ten others could
not: the same file without these two failed with redefinition errors (enum CStat / CS_COUNT in correct.h, connections.h and
components.h, enum TStat / TS_COUNT in tips.h and thread.h, C_NONE, C_BLOCK and T_NONE defined twice with different values or comments),
which is why variants.h kept private copies of the bubble rule's constants.  No GPU is needed: nothing is run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dsk_amd", "csrc")
HEADERS = ["query.h", "graph.h", "unitigs.h", "rules.h", "rowfilter.h", "tips.h", "bubbles.h", "connections.h", "variants.h", "thread.h",
           "components.h", "correct.h"]
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-ffp-contract=off"]      # (FLAGS of the Makefile)


def test_all_graph_headers_in_one_translation_unit(tmp_path):
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.skip("no hipcc")
    for h in HEADERS:
        assert os.path.exists(os.path.join(CSRC, h)), h
    src = tmp_path / "all_graph_headers.hip"
    src.write_text("#include <hip/hip_runtime.h>\n" + "".join('#include "%s"\n' % h for h in HEADERS))
    out = subprocess.run([hipcc, *FLAGS, "-fsyntax-only", "-I", CSRC, str(src)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
