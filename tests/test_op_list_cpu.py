"""csrc/common/op_list.h on CPU: what the entry points of the instruction-level diagnostics decide about an op list
and the self-check hooks before anything is launched.  The header is compiled alone with the host compiler into a
stand-alone program that walks a table of cases and prints one line per case; the expectations are written out here.
A second build of the same program runs under the host sanitizers."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from k8s_gpu_node_checker_amd import build as B

CSRC = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc", "common")

# a table of 4 ops, a grid of 8 workgroups, a step limit of 4
CASES_CPP = r"""
#include <cstdio>
#include "op_list.h"

int main() {
  constexpr int T = 4;
  const int one[] = {2}, all[] = {0, 1, 2, 3}, over[] = {0, 1, 2, 3, 0}, low[] = {1, -1}, high[] = {1, T}, twice[] = {3, 1, 3};
  printf("known null %d\n", op_list_known(nullptr, 1, T, false));
  printf("known nops0 %d\n", op_list_known(one, 0, T, false));
  printf("known one %d\n", op_list_known(one, 1, T, true));
  printf("known all %d\n", op_list_known(all, T, T, true));
  printf("known nops_over %d %d\n", op_list_known(over, T + 1, T, false), op_list_known(over, T + 1, T, true));
  printf("known index_low %d\n", op_list_known(low, 2, T, false));
  printf("known index_high %d\n", op_list_known(high, 2, T, false));
  printf("known twice distinct %d\n", op_list_known(twice, 3, T, true));
  printf("known twice any %d\n", op_list_known(twice, 3, T, false));
  printf("hook off %d\n", op_list_has_hook(twice, 3, -1));
  printf("hook off_null %d\n", op_list_has_hook(nullptr, 0, -1));
  printf("hook listed %d\n", op_list_has_hook(twice, 3, 1));
  printf("hook unlisted %d\n", op_list_has_hook(twice, 3, 2));
  printf("hook past_table %d\n", op_list_has_hook(all, T, T));
  printf("hook null_list %d\n", op_list_has_hook(nullptr, 3, 1));
  const unsigned grid = 8;
  const int limit = 4, blocks[] = {-1, 0, 7, 8}, skips[] = {-1, 0, limit - 1, limit};
  for (int b : blocks) printf("range block %d %d\n", b, hook_in_range(b, grid, -1, limit));
  for (int s : skips) printf("range skip %d %d\n", s, hook_in_range(3, grid, s, limit));
  printf("range both_out %d\n", hook_in_range(8, grid, limit, limit));
  for (int hooked = 0; hooked < 2; ++hooked)
    for (int s : {-1, 0, 2}) {
      const HookTrio h = hook_trio(hooked != 0, 5, s);
      printf("trio %d %d: %d %d %d\n", hooked, s, h.flip_block, h.skip_block, h.skip_at);
    }
  unsigned long long rec[6] = {1, 2, 3, 4, 5, 6};
  no_record(rec + 1);
  printf("record %llu %llx %llu %llu %llu %llu\n", rec[0], rec[1], rec[2], rec[3], rec[4], rec[5]);
  printf("ok\n");
  return 0;
}
"""

EXPECTED = """\
known null 0
known nops0 0
known one 1
known all 1
known nops_over 0 0
known index_low 0
known index_high 0
known twice distinct 0
known twice any 1
hook off 1
hook off_null 1
hook listed 1
hook unlisted 0
hook past_table 0
hook null_list 0
range block -1 0
range block 0 1
range block 7 1
range block 8 0
range skip -1 1
range skip 0 1
range skip 3 1
range skip 4 0
range both_out 0
trio 0 -1: -1 -1 -1
trio 0 0: -1 -1 -1
trio 0 2: -1 -1 -1
trio 1 -1: 5 -1 -1
trio 1 0: -1 5 0
trio 1 2: -1 5 2
record 1 ffffffffffffffff 0 0 0 6
ok
"""


@functools.lru_cache(maxsize=None)
def _program(sanitize):
    """op_list.h compiled with the host compiler alone into a stand-alone program; (return code, output)."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "op_list.cpp"), os.path.join(tmp, "op_list")
        with open(src, "w") as f:
            f.write(CASES_CPP)
        c = subprocess.run([cxx, *flags, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe],
                           capture_output=True, text=True)
        if c.returncode != 0:
            return None, c.stderr
        p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout + p.stderr


def test_every_case_decides_as_written_out():
    rc, out = _program(False)
    assert rc == 0, out
    assert out.splitlines() == EXPECTED.splitlines()


def test_the_cases_are_clean_under_the_host_sanitizers():
    rc, out = _program(True)
    if rc is None and re.search(r"cannot find|asan|ubsan|unrecognized", out):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert rc == 0, out
    assert out.splitlines() == EXPECTED.splitlines()


def test_the_header_has_no_hip_in_it_and_a_change_to_it_rebuilds_the_libraries_that_include_it():
    with open(os.path.join(CSRC, "op_list.h")) as f:
        assert re.findall(r"#include [<\"]([^>\"]+)", f.read()) == ["cstddef", "vector"]
    users = set()
    for name, spec in B._targets().items():
        with open(spec["sources"][0]) as f:
            includes = '#include "../common/op_list.h"' in f.read()
        assert any(h.endswith("op_list.h") for h in spec.get("headers", [])) == includes, name
        users |= {name} if includes else set()
    assert users == {"lanes", "scalar", "matrix", "vmem", "cvt", "ifetch"}
