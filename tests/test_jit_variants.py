"""Every compile-time variant of the specialised kernel, on the CPU: the table of
tests/jit_variants.py is complete, every row of it compiles for gfx950, and every row is live
(its machine code differs from the default's), so tests/test_gpu_jit_variants.py renders
kernels that are known to build and known to be variants.
"""
import os
import re
import struct

import pytest

import gen_scenes as gs
import jit_variants as jv
from csgrenderer_amd import scenes
from csgrenderer_amd import wololo as wl
from test_gen_scenes import BY_NAME, CASES, frame_params, make

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csgrenderer_amd", "csrc")
# the library kernels' device headers and the two units that instantiate them: where a library `#ifndef WO_*` may sit
LIBRARY = ("wo_tracers.h", "path_kernels.h", "query_kernels.h", "trace_kernels.hip", "query_launch.hip")
SOURCES = ("wo_device_common.h",) + LIBRARY + ("scene_jit.c",)
BEHIND = ((0.0, 4.5, 10.0), (0.0, 9.0, 20.0), (0, 1, 0), 45.0, 0.0, 10.0)  # test_gpu_sky_tiles' all-sky camera
SIZES = {"61x35": (61, 35), "13x7": (13, 7), "rank1of3": (61, 35)}


# ---- scenes and frames of the table (shared with the GPU file) ---------------------------------

def open_scene(scene, tracer=None):
    """The renderer of a table scene; environment knobs must be set before the call."""
    if scene in BY_NAME:
        return make(BY_NAME[scene], tracer)[0]
    if scene == "slabs":
        # test_gpu_parity.test_axis_parallel_rays_through_slabs: rays parallel to box faces
        r = wl.Renderer("slabs", max_nodes=64)
        front, front_planes = scenes._box_extents(r, (0.0, 0.0, -3.0), (0.5, 0.5, 0.5))
        back, _ = scenes._box_extents(r, (0.0, 0.0, 4.0), (2.0, 2.0, 0.5))
        side, side_planes = scenes._box_extents(r, (1.5, 0.0, -5.0), (0.5, 1.0, 0.5))
        r.union(wl.arg(r.union(wl.arg(front), wl.arg(back))), wl.arg(side))
        mirror, clay = r.metal((0.9, 0.9, 0.9), 0.0), r.lambertian((0.2, 0.6, 0.3))
        for pl in front_planes:
            r.set_material(pl, mirror)
        for pl in side_planes:
            r.set_material(pl, clay)
        r.set_camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 60.0, 0.0, 1.0)
    else:
        name = "csg32" if scene == "csg32_sky" else scene
        r = wl.Renderer(name, max_nodes=4096)
        scenes.build(name, r)
        if scene == "csg32_sky":
            r.set_camera(*BEHIND)
    if tracer:
        r.set_tracer(tracer)
    return r


def frame_of(scene, frame, mode):
    """The RenderParams of a table scene's frame: the row's own small frame, or a size that cuts tiles."""
    spp = 4 if mode == wl.MODE_PATHTRACE else 1
    if frame == "own" and scene in BY_NAME:
        return frame_params(mode)
    w, h = SIZES.get(frame, (33, 33) if scene == "slabs" else (64, 36))
    if scene in BY_NAME:
        return wl.render_params(w, h, spp=spp, max_depth=6, mode=mode, seed=7)
    if scene == "slabs":
        return wl.render_params(w, h, spp=spp, max_depth=4, mode=mode, seed=3)
    return wl.render_params(w, h, spp=spp, max_depth=8, mode=mode, seed=7)  # the named scenes' info.params


def variant_flags(macro, value, src, extra, needs):
    """(flags with the variant, flags of the row's default, environment of the variant)."""
    base = " ".join(f for f in (extra, needs) if f)
    if macro.startswith("WOLOLO_"):
        return base, base, {macro: str(value)}
    if value == "flip":
        default = gs.define(src, macro)
        assert default in (0, 1), (macro, default)
        value = 1 - default
    return " ".join(f for f in (base, f"-D{macro}={value}") if f), base, {}


def rows():
    """Every (macro, value, scene, flags beside it) of class variant."""
    return [(m, v, s, x) for m, e in jv.TABLE.items() if e["class"] == jv.VARIANT
            for v, s, x in e["rows"]]


def row_id(row):
    m, v, s, x = row[:4]
    return f"{m}={v}-{s}" + (("-" + x.replace("-DWO_", "").replace(" ", "+")) if x else "") + "".join(f"-{t}" for t in row[4:])


def source_of(scene, env, monkeypatch):
    """The generated source of a scene under the environment knobs `env` (none: the default)."""
    for k in ("WOLOLO_JIT_RCULL", "WOLOLO_JIT_SPATIAL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = open_scene(scene)
    src = r.jit_source()
    r.close()
    for k in env:
        monkeypatch.delenv(k)
    assert src, scene
    return src


# ---- the machine code of a code object ----------------------------------------------------------

def executable_bytes(elf):
    """The contents of an ELF64 image's executable sections (SHF_EXECINSTR), in file order."""
    assert elf[:4] == b"\x7fELF" and elf[4] == 2 and elf[5] == 1, "a little-endian ELF64 image"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    out = []
    for i in range(shnum):
        _, typ, flags, _, off, size = struct.unpack_from("<IIQQQQ", elf, shoff + i * shentsize)
        if flags & 0x4 and typ == 1:  # SHF_EXECINSTR, SHT_PROGBITS
            out.append(elf[off:off + size])
    assert out and all(out), "no executable section"
    return b"".join(out)


_TEXT = {}


def code_text(src, flags, arch, monkeypatch):
    """(executable bytes, key) of the source's code object under WOLOLO_JIT_FLAGS=flags, read
    from the on-disk cache entry the build wrote (48 bytes of header, then the image)."""
    if flags:
        monkeypatch.setenv("WOLOLO_JIT_FLAGS", flags)
    else:
        monkeypatch.delenv("WOLOLO_JIT_FLAGS", raising=False)
    key = wl.jit_code_object(src, arch)[3]
    if key not in _TEXT:
        with open(os.path.join(os.environ["WOLOLO_JIT_CACHE"], key + ".co"), "rb") as f:
            blob = f.read()
        assert blob[:8] == b"WOJITCO1"
        _TEXT[key] = executable_bytes(blob[48:])
    return _TEXT[key], key


@pytest.fixture(scope="module")
def cache_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("jit_variants_cache")
    os.chmod(d, 0o700)
    return str(d)


@pytest.fixture()
def cache(cache_dir, monkeypatch, hostonly):
    """One empty code-object cache for this file's builds: every entry read here was built here."""
    monkeypatch.setenv("WOLOLO_JIT_CACHE", cache_dir)
    return cache_dir


# ---- completeness --------------------------------------------------------------------------------

FORM_ROWS = ("flat_w1", "dl_lut", "lut_long_term", "chain_33", "hlut_regs", "hlut_4w", "term_64", "pairs_65", "ties_nest")


def _guarded(text):
    return set(re.findall(r"#\s*ifndef\s+(WO_[A-Z0-9_]+)", text))


def test_the_table_names_every_switch(hostonly, monkeypatch):
    """Every `#ifndef WO_*` of the sources and of the generated text of the named scenes
    and of one row per form has an entry, and every entry's macro still exists."""
    found = set()
    for f in SOURCES:
        with open(os.path.join(CSRC, f)) as fh:
            found |= _guarded(fh.read())
    assert {frozenset(BY_NAME[n].want["forms"]) for n in FORM_ROWS} == {frozenset(c.want["forms"]) for c in CASES}
    for scene in ("csg32", "csg32_nested", "csg256_chain") + FORM_ROWS:
        found |= _guarded(source_of(scene, {}, monkeypatch))
    macros = {m for m in jv.TABLE if m.startswith("WO_")}
    assert found - macros == set(), "switches without an entry in tests/jit_variants.py"
    assert macros - found == set(), "entries whose macro is gone"
    static = set()
    for f in LIBRARY:
        with open(os.path.join(CSRC, f)) as fh:
            static |= _guarded(fh.read())
    for m, e in jv.TABLE.items():
        assert e["class"] in (jv.VARIANT, jv.INSTRUMENTATION, jv.LIBRARY_BUILD), m
        if e["class"] == jv.LIBRARY_BUILD:
            assert m in static, m
        if e["class"] != jv.VARIANT:
            assert e["reason"], m
    assert set(jv.ALSO_LIBRARY_BUILD) <= static


def test_the_table_names_every_source_knob():
    with open(os.path.join(CSRC, "scene_jit.c")) as fh:
        knobs = set(re.findall(r'getenv\("(WOLOLO_JIT_[A-Z0-9_]+)"\)', fh.read()))
    listed = {m for m in jv.TABLE if m.startswith("WOLOLO_")}
    assert knobs - listed - set(jv.KNOBS_TESTED_ELSEWHERE) == set()
    assert listed - knobs == set(), "entries whose knob is gone"


def test_every_variant_has_a_row():
    for m, e in jv.TABLE.items():
        if e["class"] == jv.VARIANT:
            assert e["rows"] and e["frames"], m
            for _, s, _ in e["rows"]:
                assert s in BY_NAME or s in scenes.SCENES or s in ("slabs", "csg32_sky"), (m, s)
            assert set(e["frames"]) <= {"own"} | set(SIZES), m


def test_axis_pairs_are_where_the_table_says(hostonly):
    """Half-space leaves with u1 != 0 are the axis-aligned ones (test_scene_compile.py): the named
    scenes and the slabs have them, so WO_AXIS_PAIR_* is tested there; which generated rows have
    none is printed, and the liveness test below is what decides a row's place in the table."""
    def axis_leaves(scene):
        r = open_scene(scene)
        prog, nrec, _ = r.program()
        n = sum(1 for pc in range(nrec) if prog[pc].op == wl.WO_LEAF_HALFSPACE and prog[pc].u1 != 0)
        r.close()
        return n

    for _, s, _ in jv.TABLE["WO_AXIS_PAIR_OPAQUE"]["rows"]:
        assert axis_leaves(s) >= 2, s
    print({c.name: axis_leaves(c.name) for c in CASES})


def test_sky_scene_is_all_sky(hostonly):
    """`csg32_sky` is what its name says: the oracle traces one segment per sample."""
    import pyoracle

    r = open_scene("csg32_sky")
    p = frame_of("csg32_sky", "own", wl.MODE_PATHTRACE)
    prog, nrec, _ = r.program()
    mats, nm = r.materials()
    segs = pyoracle.pathtrace_rows(prog, nrec, mats, nm, r.frame_desc(p), 0, p.height)[1]
    r.close()
    assert segs == p.width * p.height * p.spp


# ---- every row compiles, and is live -------------------------------------------------------------

@pytest.mark.parametrize("row", rows(), ids=row_id)
def test_variant_compiles_and_is_live(cache, monkeypatch, row):
    """The row's code object builds for gfx950 (a failure shows the compiler's log here, never
    first on a GPU machine) and its executable bytes differ from those of the same source (the
    knobs: the default source) under the row's other flags alone."""
    macro, value, scene, extra = row
    e = jv.TABLE[macro]
    src0 = source_of(scene, {}, monkeypatch)
    flags, base, env = variant_flags(macro, value, src0, extra, e["needs"])
    src = source_of(scene, env, monkeypatch) if env else src0
    if env:
        # a knob rewrites the text, and the scene keeps its forms
        assert src != src0 and gs.forms(src) == gs.forms(src0), row
    text0, key0 = code_text(src0, base, "gfx950", monkeypatch)
    text, key = code_text(src, flags, "gfx950", monkeypatch)
    print(row_id(row), "scratch, LDS", wl.jit_code_resources(src, "gfx950"), "default",
          _default_resources(src0, base, monkeypatch), len(text), "B of code, default", len(text0))
    assert key != key0
    assert text != text0, f"{row_id(row)}: the machine code is the default's -- the variant does not act on this scene"


def _default_resources(src, base, monkeypatch):
    if base:
        monkeypatch.setenv("WOLOLO_JIT_FLAGS", base)
    else:
        monkeypatch.delenv("WOLOLO_JIT_FLAGS", raising=False)
    return wl.jit_code_resources(src, "gfx950")


def test_a_misspelt_flag_is_the_default_code(cache, monkeypatch):
    """The negative of the liveness test: a macro nothing reads gives a new key and the same code."""
    src = source_of("one_prim", {}, monkeypatch)
    text0, key0 = code_text(src, "", "gfx950", monkeypatch)
    text, key = code_text(src, "-DWO_NO_SUCH_SWITCH=1", "gfx950", monkeypatch)
    assert key != key0 and text == text0


def test_camera_wave_mode_2_is_refused(cache, monkeypatch):
    """WO_CAM_WAVES once had a mode 2; pathtrace_block now states its modes in a static_assert,
    so the stale value fails to build instead of silently rendering as another mode."""
    src = source_of("one_prim", {}, monkeypatch)
    monkeypatch.setenv("WOLOLO_JIT_FLAGS", "-w -DWO_CAM_WAVES=2")  # (-w: the log begins with the error)
    with pytest.raises(wl.WololoError, match="camera-wave modes"):
        wl.jit_code_object(src, "gfx950")


# ---- the host harness of the root evaluation ------------------------------------------------------

def test_no_further_variant_reaches_the_host_evaluated_text(hostonly, monkeypatch):
    """test_jit.py / test_gen_scenes.py compile the text between the WO_EVAL and WO_TOGGLE marks on
    the host under both values of WO_JIT_LUT and WO_HBITS_LDS.  Those two are the only switches
    of the table that text reads: a new one there must join the harness."""
    names = [m for m in jv.TABLE if m.startswith("WO_")]
    for scene in ("csg32_nested", "csg256_chain") + tuple(c.name for c in CASES):
        src = source_of(scene, {}, monkeypatch)
        if "// WO_EVAL_BEGIN" not in src:
            continue
        text = (src[src.index("// WO_EVAL_BEGIN"):src.index("// WO_EVAL_END")]
                + src[src.index("// WO_TOGGLE_BEGIN"):src.index("// WO_TOGGLE_END")])
        used = {m for m in names if re.search(r"\b" + m + r"\b", text)}
        assert used <= {"WO_JIT_LUT", "WO_HBITS_LDS"}, (scene, used)
