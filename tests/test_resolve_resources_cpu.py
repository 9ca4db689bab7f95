"""Register budget of k_resolve (kernels_resolve.h), checked without a GPU: a device-only compile of topo_kernels.hip, the one
device translation unit, with the Makefile's flags, read back from the code object's metadata.
k_resolve is bound by instruction issue, and every spilled register costs issue
slots (v_writelane / v_readlane, scratch traffic) in the loops around the rows; these ceilings keep a change from quietly
bringing the spills back."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "topo-renderer_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.environ.get("HIPCC", os.path.join(ROCM, "bin", "hipcc"))
LLVM = os.path.join(ROCM, "lib", "llvm", "bin")

# per instantiation of k_resolve: at most this many SGPRs spilled (to VGPR lanes) and bytes of scratch per lane; no VGPR spills
MAX_SGPR_SPILLS = 16
MAX_SCRATCH_BYTES = 28          # two stores of a private temporary in the triangle setup (never read back); no spill slots
LDS_PER_CU = 160 * 1024


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    flags = re.search(r"^FLAGS = (.*)$", text, re.M).group(1).replace("$(ARCH)", arch)
    return arch, flags.split()


def _resolve_wgs():
    src = open(os.path.join(CSRC, "kernels_resolve.h")).read()
    return int(re.search(r"^#define TOPO_RESOLVE_WGS (\d+)", src, re.M).group(1))


def _kernels(notes):
    """The code-object notes as {kernel symbol: {field: value}} (the AMDHSA metadata YAML, one kernel per '- .' block)."""
    out, cur = {}, None
    for line in notes.split("\n"):
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(.*)", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2).strip()
        if line.lstrip().startswith("- .") and key in ("agpr_count", "args"):
            cur = {}
        if cur is None:
            continue
        cur[key] = val
        if key == "name":
            out[val] = cur
    return out


@pytest.fixture(scope="module")
def resolve_kernels(tmp_path_factory):
    for tool in (HIPCC, os.path.join(LLVM, "clang-offload-bundler"), os.path.join(LLVM, "llvm-readelf")):
        if not (os.path.exists(tool) or shutil.which(tool)):
            pytest.fail(f"{tool} is needed to compile the HIP library and is missing")
    arch, flags = _makefile_flags()
    tmp = tmp_path_factory.mktemp("resolve_resources")
    dev, obj = str(tmp / "dev.o"), str(tmp / f"{arch}.o")
    subprocess.check_call([HIPCC, *[f for f in flags if f != "-Wall"], "--cuda-device-only", "-c", "-o", dev,
                           os.path.join(CSRC, "topo_kernels.hip")], cwd=str(tmp))
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={dev}",
                           f"--targets=hip-amdgcn-amd-amdhsa--{arch}", f"--output={obj}"])
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], text=True)
    ks = {name: k for name, k in _kernels(notes).items() if "k_resolve" in name}
    assert len(ks) == 4, f"expected the four k_resolve instantiations, found {sorted(ks)}"
    return ks


def test_resolve_has_no_vgpr_spills(resolve_kernels):
    for name, k in resolve_kernels.items():
        assert int(k.get("vgpr_spill_count", "0")) == 0, (name, k.get("vgpr_spill_count"))


def test_resolve_sgpr_spills_within_ceiling(resolve_kernels):
    for name, k in resolve_kernels.items():
        assert int(k.get("sgpr_spill_count", "0")) <= MAX_SGPR_SPILLS, (name, k.get("sgpr_spill_count"))


def test_resolve_scratch_within_ceiling(resolve_kernels):
    for name, k in resolve_kernels.items():
        assert int(k["private_segment_fixed_size"]) <= MAX_SCRATCH_BYTES, (name, k["private_segment_fixed_size"])


def test_resolve_lds_fits_its_workgroups_per_cu(resolve_kernels):
    wgs = _resolve_wgs()
    for name, k in resolve_kernels.items():
        assert int(k["group_segment_fixed_size"]) * wgs <= LDS_PER_CU, (name, k["group_segment_fixed_size"], wgs)
