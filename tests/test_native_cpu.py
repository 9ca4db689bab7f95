"""tests/native.py, the builder of the TEST-ONLY g++ code: it rebuilds when a header that only another header includes changes, when
the flags change, and not otherwise; a compile that fails leaves the last good output in place."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import native


@pytest.fixture
def tree(tmp_path):
    """a.cpp includes a.h, which includes b.h, and b.h defines the constant answer() returns."""
    (tmp_path / "a.cpp").write_text('#include "a.h"\nextern "C" int answer() { return ANSWER + X; }\n')
    (tmp_path / "a.h").write_text('#include "b.h"\n#ifndef X\n#define X 0\n#endif\n')
    (tmp_path / "b.h").write_text("#define ANSWER 41\n")
    return tmp_path


def _build(tree, **kw):
    return native.build("liba.so", [str(tree / "a.cpp")], out_dir=str(tree / "out"), **kw)


def _answer(so, tree, n=[0]):
    n[0] += 1      # (a copy under a fresh name: the loader hands back the library it already holds for a name it knows)
    return C.CDLL(shutil.copy(so, str(tree / f"loaded{n[0]}.so"))).answer()


def _identity(so):
    st = os.stat(so)
    return st.st_mtime_ns, st.st_ino


def test_second_build_compiles_nothing(tree):
    so = _build(tree)
    assert _answer(so, tree) == 41
    first = _identity(so)
    assert _build(tree) == so and _identity(so) == first
    assert sorted(os.listdir(tree / "out")) == ["liba.so", "liba.so.cmd", "liba.so.d"], "no temporary file is left behind"


def test_header_of_a_header_rebuilds(tree):
    so = _build(tree)
    first = _identity(so)
    assert {os.path.basename(d) for d in native.deps("liba.so", str(tree / "out"))} == {"a.cpp", "a.h", "b.h"}
    (tree / "b.h").write_text("#define ANSWER 17\n")
    later = os.stat(so).st_mtime_ns + 10 ** 9
    os.utime(tree / "b.h", ns=(later, later))
    assert _build(tree) == so and _identity(so) != first
    assert _answer(so, tree) == 17
    os.utime(so, ns=(later, later))      # (the output is no older than b.h now)
    again = _identity(so)
    _build(tree)
    assert _identity(so) == again


def test_other_flags_rebuild(tree):
    so = _build(tree)
    first = _identity(so)
    assert _build(tree, flags=native.DEFAULT_FLAGS + ("-DX=1",)) == so and _identity(so) != first
    assert _answer(so, tree) == 42
    again = _identity(so)
    _build(tree, flags=native.DEFAULT_FLAGS + ("-DX=1",))
    assert _identity(so) == again


def test_failed_compile_keeps_the_last_good_output(tree):
    so = _build(tree)
    first = _identity(so)
    (tree / "a.cpp").write_text('#include "a.h"\nextern "C" int answer() { return no_such_name; }\n')
    later = os.stat(so).st_mtime_ns + 10 ** 9
    os.utime(tree / "a.cpp", ns=(later, later))
    with pytest.raises(subprocess.CalledProcessError):
        _build(tree)
    assert _identity(so) == first and _answer(so, tree) == 41
    assert sorted(os.listdir(tree / "out")) == ["liba.so", "liba.so.cmd", "liba.so.d"]
    with pytest.raises(subprocess.CalledProcessError):      # still stale: the next call tries again
        _build(tree)


def test_a_program_builds_and_runs(tree):
    (tree / "a.cpp").write_text('#include "a.h"\nint main() { return ANSWER; }\n')
    exe = native.build("a_prog", [str(tree / "a.cpp")], shared=False, out_dir=str(tree / "out"))
    assert subprocess.run([exe]).returncode == 41


def test_emulations_depend_on_the_srgb_tables():
    """cover_emul.cpp, los_emul.cpp and surface_emul.cpp reach srgb_tables.h through topo_pipeline.h only."""
    import cover_emul
    import los_emul
    import surface_emul
    for mod, name in ((cover_emul, "libcover_emul.so"), (los_emul, "liblos_emul.so"), (surface_emul, "libsurface_emul.so")):
        mod.lib()
        assert "srgb_tables.h" in {os.path.basename(d) for d in native.deps(name)}, name
