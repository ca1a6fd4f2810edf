"""tests/emu/_emu.py, the emulators' one build-and-bind path, on a three-line source in a temporary directory: a library is rebuilt when,
and only when, its command or the content of something the command can read has changed; a failed build leaves nothing to load."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import support                          # noqa: F401  (its import puts tests/emu, where _emu lives, on the path)
import _emu

SOURCE = '#include "answer.h"\n#include "other.h"\nextern "C" int answer() { return ANSWER + SHIFT + OTHER; }\n'


def _write(path, text):
    with open(path, "w") as fh:
        fh.write(text)


@pytest.fixture
def tree(tmp_path):
    """(source, where): an include/ and a hip/ root and an output directory under tmp_path, as shared_lib's keywords"""
    inc, hip, out = tmp_path / "include", tmp_path / "hip", tmp_path / "out"
    for d in (inc, hip, out):
        d.mkdir()
    _write(inc / "answer.h", "#define ANSWER 40\n")
    _write(hip / "other.h", "#define OTHER 0\n")
    _write(tmp_path / "three.cpp", SOURCE)
    where = {"incs": (str(inc), str(hip)), "roots": ((str(inc), "*"), (str(hip), "*.h")), "out_dir": str(out)}
    return str(tmp_path / "three.cpp"), where


def _stamp(path):
    st = os.stat(path)
    return st.st_ino, st.st_mtime_ns


def _rebuilt(call, lib):
    before = _stamp(lib)
    assert call() == lib
    return _stamp(lib) != before


def test_a_library_is_rebuilt_when_and_only_when_its_key_changes(tree):
    src, where = tree
    inc = where["incs"][0]
    lib = _emu.lib_path("three", where["out_dir"])

    def build(opt="-O2", defines=("SHIFT=2",)):
        return _emu.build_lib("three", [src], opt, defines, **where)

    h = _emu.shared_lib("three", [src], "-O2", ("SHIFT=2",), {"answer": (C.c_int, [])}, **where)
    assert h.answer() == 42 and h.answer.restype is C.c_int and os.path.exists(lib)
    # (a) neither a second shared_lib nor a second build compiles: the same file, untouched
    before = _stamp(lib)
    assert _emu.shared_lib("three", [src], "-O2", ("SHIFT=2",), {"answer": (C.c_int, [])}, **where) is h
    assert not _rebuilt(build, lib) and _stamp(lib) == before
    assert sorted(os.listdir(where["out_dir"])) == ["build", "libthree.so"]                 # (no temporary left)
    # (b) a header's content changes, its mtime does not (tests/test_abi.py does this to include/prt_types.h)
    header = os.path.join(inc, "answer.h")
    st = os.stat(header)
    _write(header, "#define ANSWER 41\n")
    os.utime(header, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert _rebuilt(build, lib) and not _rebuilt(build, lib)
    # (c) only a define, or only the optimisation level
    assert _rebuilt(lambda: build(defines=("SHIFT=3",)), lib) and not _rebuilt(lambda: build(defines=("SHIFT=3",)), lib)
    assert _rebuilt(lambda: build(opt="-O1", defines=("SHIFT=3",)), lib)
    assert _rebuilt(lambda: build(opt=("-O1", "-fno-slp-vectorize"), defines=("SHIFT=3",)), lib)
    assert _rebuilt(build, lib) and not _rebuilt(build, lib)
    # (d) a new header under a keyed root, named in no list
    _write(os.path.join(where["roots"][1][0], "new.h"), "// nothing includes this yet\n")
    assert _rebuilt(build, lib) and not _rebuilt(build, lib)
    _write(os.path.join(where["roots"][1][0], "not_a_header.txt"), "the second root is keyed by *.h\n")
    assert not _rebuilt(build, lib)
    # what is loaded is what the last build made (a fresh process: this one keeps the first handle of the path)
    r = subprocess.run([sys.executable, "-c", "import ctypes, sys; sys.exit(ctypes.CDLL(sys.argv[1]).answer())", lib])
    assert r.returncode == 41 + 2


def test_a_failed_build_leaves_nothing_a_later_call_would_accept(tree, capfd):
    src, where = tree
    out = where["out_dir"]
    _write(src, SOURCE + "this is no C++\n")
    with pytest.raises(subprocess.CalledProcessError):
        _emu.build_lib("three", [src], "-O2", ("SHIFT=2",), **where)
    capfd.readouterr()                                    # (the compiler's complaint)
    assert [f for f in os.listdir(out) if f != "build"] == [] and os.listdir(os.path.join(out, "build")) == []
    with pytest.raises(subprocess.CalledProcessError):    # ... so the next call compiles again, and fails again
        _emu.build_lib("three", [src], "-O2", ("SHIFT=2",), **where)
    capfd.readouterr()
    # a good library before the failure is not taken for the broken source's either
    _write(src, SOURCE)
    lib = _emu.build_lib("three", [src], "-O2", ("SHIFT=2",), **where)
    _write(src, SOURCE + "this is no C++\n")
    with pytest.raises(subprocess.CalledProcessError):
        _emu.build_lib("three", [src], "-O2", ("SHIFT=2",), **where)
    capfd.readouterr()
    _write(src, SOURCE)
    assert not _rebuilt(lambda: _emu.build_lib("three", [src], "-O2", ("SHIFT=2",), **where), lib)      # (the old pair still stands for the old source)
