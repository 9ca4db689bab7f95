"""tools/exp_build.sh lists the library's sources by hand: they must be the Makefile's SRCS, or every experiment library lacks a
unit's launchers and cannot be loaded (ctypes opens it with RTLD_NOW)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = re.compile(r"\b\w+\.(?:hip|cpp)\b")


def test_experiment_builds_compile_the_makefiles_sources():
    make = open(os.path.join(ROOT, "topo-renderer_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    assert "topo_kernels.hip" in srcs and "terrain_queries.cpp" in srcs
    script = open(os.path.join(ROOT, "tools", "exp_build.sh")).read()
    line = [l for l in script.split("\n") if "-shared" in l]
    assert len(line) == 1
    assert sorted(SOURCE.findall(line[0])) == sorted(srcs)
