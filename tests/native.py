"""The one place that runs g++ for test code: the TEST-ONLY builds of the product's headers (tests/*_emul.cpp, prefilter_shim.cpp,
limits_emul.cpp) into tests/_build, rebuilt when a file the compiler itself named as a dependency is newer than the output."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_MATH = "../topo-renderer_amd/csrc/host_math.cpp"      # the product's CPU math, linked by the builds that read its tables
BUILD_DIR = os.path.join(HERE, "_build")
DEFAULT_FLAGS = ("-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma")


def deps(name, out_dir=BUILD_DIR) -> list:
    """The files the compiler read for the last build of `name` (its sources and every header they reach, system headers left out)."""
    with open(os.path.join(out_dir, name + ".d")) as f:
        words = f.read().replace("\\\n", " ").split()
    return [os.path.normpath(os.path.join(out_dir, w)) for w in words if not w.endswith(":")]


def _stale(out, name, out_dir, cmd):
    try:
        with open(out + ".cmd") as f:
            if f.read() != cmd:
                return True
        built = os.stat(out).st_mtime_ns
        return any(os.stat(d).st_mtime_ns > built for d in deps(name, out_dir))
    except OSError:      # no output, no depfile, no saved command line, or a dependency that is gone
        return True


def _replace(text, path, tmp):
    with open(os.path.join(tmp, "text"), "w") as f:
        f.write(text)
    os.replace(f.name, path)


def build(name, sources, *, flags=DEFAULT_FLAGS, shared=True, out_dir=BUILD_DIR) -> str:
    """g++ of `sources` into out_dir/name, a shared library or (shared=False) a program; -> its path.  Every step writes into a
    folder of its own beside the output, and the linked output is moved onto its name: a reader sees the old file or the new
    one, a failed compile leaves the old one.  g++ runs in out_dir on names relative to it, so the saved command line and the depfile
    stay true when the tree is copied elsewhere."""
    out = os.path.join(out_dir, name)
    sources = [os.path.relpath(os.path.join(HERE, s), out_dir) for s in sources]      # (relative names: from this folder)
    link = ["g++", *flags] + (["-shared"] if shared else [])
    cmd = " ".join(link + sources)
    if not _stale(out, name, out_dir, cmd):
        return out
    os.makedirs(out_dir, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix=name + ".", dir=out_dir)
    try:
        objs = [os.path.join(tmp, f"{i}.o") for i in range(len(sources))]
        for src, obj in zip(sources, objs):      # (one depfile per source: a second source would overwrite the first's)
            subprocess.check_call(["g++", *flags, "-MMD", "-MF", obj + ".d", "-MT", name, "-c", src, "-o", obj], cwd=out_dir)
        subprocess.check_call(link + ["-o", os.path.join(tmp, name)] + objs, cwd=out_dir)
        text = ""
        for obj in objs:
            with open(obj + ".d") as f:
                text += f.read()
        os.replace(os.path.join(tmp, name), out)
        _replace(text, out + ".d", tmp)
        _replace(cmd, out + ".cmd", tmp)      # (last: an output without its command line counts as stale)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def load(name, sources, restypes):
    """build() and load the shared library `name`; restypes: {function: its ctypes result type}."""
    lib = C.CDLL(build(name, sources))
    for fn, restype in restypes.items():
        getattr(lib, fn).restype = restype
    return lib
