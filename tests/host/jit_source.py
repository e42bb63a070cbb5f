"""A generated specialised-kernel source for the code-object pipeline's stand-alone driver
(jit_code_main.cpp): python tests/host/jit_source.py OUT.hip writes the source of the
two-sphere difference scene (test_jit.py's cache test scene).  No GPU needed."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
os.environ.setdefault("WOLOLO_ALLOW_NO_DEVICE", "1")

from csgrenderer_amd import wololo as wl  # noqa: E402

if __name__ == "__main__":
    r = wl.Renderer("two-spheres", max_nodes=64)
    a = r.sphere(0.5)
    b = r.sphere(0.3)
    r.difference(wl.arg(a), wl.arg(b, (0.2, 0.0, 0.0)))
    with open(sys.argv[1], "w") as f:
        f.write(r.jit_source())
    r.close()
