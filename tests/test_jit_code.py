"""The specialised kernels' code-object pipeline (csrc/jit_code.cpp) through its stand-alone
driver (tests/host/jit_code_main.cpp), built without sanitizers: the kernel-descriptor
reader over a real code object, its prefixes and its header fields set to hostile values;
the process cache's bound and order; a helper that yields no object.  No GPU: hiprtc
compiles for gfx950 anywhere.  `make -C csgrenderer_amd/csrc jit-code-asan` runs the same
program under ASan and UBSan."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csgrenderer_amd", "csrc")


def test_code_object_pipeline_driver(tmp_path):
    subprocess.run(["make", "-C", CSRC, "jit-code-driver"], check=True, stdout=subprocess.DEVNULL)
    src = tmp_path / "two_spheres.hip"
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host", "jit_source.py"), str(src)], check=True)
    cache = tmp_path / "cache"
    cache.mkdir()
    run = subprocess.run([os.path.join(ROOT, "csgrenderer_amd", "build", "jit_code_driver"),
                          os.path.join(ROOT, "csgrenderer_amd", "lib", "wo_jitc"), str(cache), str(src)],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "descriptor reader:" in run.stdout and "process cache:" in run.stdout and "helper fallback:" in run.stdout
    assert len(list(cache.glob("*.co"))) == 2  # the in-process compiler's object and the helper's
