"""The library kernels' identity (the Makefile's static_key.inc, WO_STATIC_SRC_SHA) names the kernels'
device sources, the flags and the compiler -- not the host code round them.  CPU only: a copy of
csrc/ and include/ in a temporary directory, where nothing but static_key.inc is made."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_FILES = ("trace_kernels.hip", "query_launch.hip", "wo_dev_impl.h", "wo_dev.h")
UNITS = ("trace_kernels.hip", "query_launch.hip", "denoise_kernels.hip")  # they instantiate and launch; the denoiser has no key


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    top = tmp_path_factory.mktemp("static_key")
    shutil.copytree(os.path.join(ROOT, "csgrenderer_amd", "csrc"), top / "csgrenderer_amd" / "csrc")
    shutil.copytree(os.path.join(ROOT, "include"), top / "include")
    return top


def _make(tree, *args):
    csrc, obj = tree / "csgrenderer_amd" / "csrc", tree / "obj"
    return subprocess.run(["make", "-C", str(csrc), f"OBJ_DIR={obj}", *args], check=True, capture_output=True,
                          text=True).stdout


def _key(tree):
    _make(tree, str(tree / "obj" / "static_key.inc"))
    with open(tree / "obj" / "static_key.inc") as fh:
        m = re.fullmatch(r'#define WO_STATIC_SRC_SHA "([0-9a-f]{64})"\n', fh.read())
    assert m, "static_key.inc is not one define of a SHA-256"
    return m.group(1)


def _key_srcs(tree):
    """KEY_SRCS as make expands it: paths relative to csrc/, or absolute."""
    csrc = tree / "csgrenderer_amd" / "csrc"
    with open(csrc / "print_key_srcs.mk", "w") as fh:
        fh.write("include Makefile\nprint-key-srcs:\n\t@echo $(KEY_SRCS)\n")
    try:
        out = subprocess.run(["make", "-s", "-C", str(csrc), "-f", "print_key_srcs.mk", f"OBJ_DIR={tree / 'obj'}",
                              "print-key-srcs"], check=True, capture_output=True, text=True).stdout
    finally:
        os.remove(csrc / "print_key_srcs.mk")
    return [os.path.normpath(os.path.join(csrc, p)) for p in out.split()]


def _with_a_comment(path, key_of):
    """The key with one comment line appended to `path`; the file is put back."""
    with open(path, "rb") as fh:
        before = fh.read()
    try:
        with open(path, "ab") as fh:
            fh.write(b"\n// a comment\n")
        return key_of()
    finally:
        with open(path, "wb") as fh:
            fh.write(before)


def test_host_edits_leave_the_key(tree):
    key = _key(tree)
    for f in HOST_FILES:
        path = tree / "csgrenderer_amd" / "csrc" / f
        assert os.path.exists(path), f
        assert _with_a_comment(path, lambda: _key(tree)) == key, f"{f} is host code but moves the kernels' identity"
    assert _key(tree) == key


def test_every_key_source_moves_the_key(tree):
    key = _key(tree)
    srcs = _key_srcs(tree)
    assert len(srcs) >= 5
    for path in srcs:
        assert _with_a_comment(path, lambda: _key(tree)) != key, f"{path} is in KEY_SRCS but does not move the key"
    assert _key(tree) == key


def _includes(path):
    with open(path) as fh:
        return re.findall(r'^\s*#\s*include\s+"([^"]+)"', fh.read(), re.M)


def test_the_key_covers_the_kernels_sources(tree):
    """Every HIP source of csrc/ with a __global__ in it (the units apart), and every project header
    those reach through #include "...", is in KEY_SRCS.  (scene_jit.c, a C file, has one in the text
    it emits for the specialised kernel, whose identity is its own key.)"""
    csrc, inc = tree / "csgrenderer_amd" / "csrc", tree / "include"
    srcs = set(_key_srcs(tree))
    todo = []
    for f in sorted(os.listdir(csrc)):
        if f in UNITS or not f.endswith((".h", ".hip")):
            continue
        with open(csrc / f, errors="replace") as fh:
            if "__global__" in fh.read():
                todo.append(os.path.normpath(csrc / f))
    assert todo, "no kernel source found"
    seen = set()
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.add(path)
        assert path in srcs, f"{os.path.relpath(path, tree)} holds or feeds kernel code but is not in KEY_SRCS"
        for name in _includes(path):
            hits = [os.path.normpath(d / name) for d in (csrc, inc) if os.path.exists(d / name)]
            assert hits or name.endswith(".inc"), f"{path} includes {name}, which is not in the tree"
            todo += hits
