"""Light updates at the C ABI and in the Python mirror: the four symbols, the struct layouts they leave alone, scene.with_lighting and
scene.light_changes, and what the CLI refuses — everything that needs no device."""
import ctypes as C
import os

import pytest

from loltracer_amd import gpu, scene as S
from loltracer_amd.__main__ import main as cli_main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
SYMBOLS = ("lol_gpu_light_update_rays", "lol_gpu_light_update_pixels", "lol_gpu_relight_held", "lol_gpu_relight_views_held")


def test_the_four_symbols_exist_and_refuse_a_null_context(scenes):
    lib = gpu.gpu_lib()
    for name in SYMBOLS:
        assert name in gpu.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    passes, relit, fc = gpu.LightPasses(), gpu.Relit(), S.FrameCamera()
    look = scenes["scene4"].flatten()
    assert lib.lol_gpu_light_update_rays(None, C.byref(look), None, 0, 1, 0, C.byref(passes), None) == -3
    assert lib.lol_gpu_light_update_pixels(None, C.byref(look), C.byref(fc), 8, 8, None, 64, 1, 2, C.byref(passes), None) == -3
    assert lib.lol_gpu_relight_held(None, C.byref(look), C.byref(look), C.byref(passes), 0, C.byref(relit), None) == -3
    assert lib.lol_gpu_relight_held(None, None, None, C.byref(passes), 0, C.byref(relit), None) == -3
    assert lib.lol_gpu_relight_views_held(None, C.byref(look), C.byref(look), C.byref(passes), 1, 2, 8, 8, 2, C.byref(relit), None) == -3
    assert lib.lol_gpu_relight_views_held(None, None, None, C.byref(passes), 1, 2, 8, 8, 2, C.byref(relit), None) == -3


def test_the_structs_are_what_they_were():
    vp = C.sizeof(C.c_void_p)
    assert C.sizeof(gpu.LightFactor) == 16 and gpu.LightFactor.specular_incidence.offset == 8        # the 4 bytes a specular update writes
    assert C.sizeof(gpu.LightPasses) == 4 * vp + C.sizeof(C.c_size_t)
    assert C.sizeof(gpu.Relit) == 3 * vp
    hdr = open(os.path.join(ROOT, "include", "lol_gpu.h")).read()
    for name in SYMBOLS:
        assert hdr.count(name + "(") >= 1, name


def test_the_update_is_the_interpreters_alone():
    """like the capture: no scene module includes the update's header"""
    src = open(os.path.join(ROOT, "loltracer_amd", "csrc", "lol_codegen.hip")).read()
    assert "lol_kernel_light_update.h" not in src and "light_update_interp" not in src
    mk = open(os.path.join(ROOT, "loltracer_amd", "csrc", "Makefile")).read()
    assert "lol_kernel_light_update.h" in mk.split("AOT_HDRS :=")[1].split("\n")[0]


# ------------------------------------------------------------------------------------------------------ with_lighting, light_changes
def bits(v3):
    return bytes(memoryview(v3).cast("B"))


@pytest.mark.parametrize("name", ["scene4", "scene", "three_lights"])
def test_with_lighting_replaces_points_and_shininess_alone(scenes, name):
    sc = scenes[name] if name in scenes else S.Scene.parse_file(os.path.join(SCENES, name + ".lol"))
    nl, nm = len(sc.lights()), len(sc.materials())
    assert S.light_changes(sc, sc.with_lighting()) == (0, 0) and sc.with_lighting().tables() == sc.tables()
    pts = [None] * nl
    pts[nl - 1] = (1.5, float("inf"), -0.0)
    moved = sc.with_lighting(points=pts)
    assert moved.lights()[nl - 1].point.tuple() == (1.5, float("inf"), -0.0)
    for l in range(nl):
        assert bits(moved.lights()[l].diffuse_intensity) == bits(sc.lights()[l].diffuse_intensity)
        assert (bits(moved.lights()[l].point) == bits(sc.lights()[l].point)) == (l != nl - 1)
    assert S.geometry_difference(sc, moved) is not None and S.geometry_difference(sc, moved, lighting=False) is None
    assert S.light_changes(sc, moved) == (1 << (nl - 1), 0)
    assert S.light_changes(moved, sc) == (1 << (nl - 1), 0)
    shiny = sc.with_lighting(shininess=[None] * (nm - 1) + [77.0])
    assert shiny.materials()[nm - 1].shininess == 77.0 and bits(shiny.materials()[nm - 1].diffuse) == bits(sc.materials()[nm - 1].diffuse)
    assert S.light_changes(sc, shiny) == (0, (1 << nl) - 1)                 # every light's specular incidence, no march
    both = moved.with_lighting(shininess=[3.0] * nm)
    assert S.light_changes(sc, both) == (1 << (nl - 1), ((1 << nl) - 1) & ~(1 << (nl - 1)))
    # a look in the sense of relighting changes neither mask
    assert S.light_changes(sc, sc.with_look(ambient=(.5, .5, .5), lights=[((1, 2, 3), (3, 2, 1))] * nl)) == (0, 0)
    # shininess is compared as bits: a NaN equals itself, and -0 differs from +0
    nan = sc.with_lighting(shininess=[float("nan")] * nm)
    assert S.light_changes(nan, nan.clone()) == (0, 0)
    assert S.light_changes(sc.with_lighting(shininess=[0.0] * nm), sc.with_lighting(shininess=[-0.0] * nm))[1] == (1 << nl) - 1
    with pytest.raises(ValueError):
        sc.with_lighting(points=[None] * (nl + 1))
    with pytest.raises(ValueError):
        sc.with_lighting(shininess=[None] * (nm + 1))


def test_light_changes_raises_with_the_reason(scenes):
    sc = scenes["scene4"]
    grown = sc.clone()
    node = next(grown.c.nodes[i] for i in range(grown.c.n_nodes) if grown.c.nodes[i].type == S.NODE_SPHERE)
    node.radius *= 1.5
    with pytest.raises(ValueError, match="differs in a number"):
        S.light_changes(sc, grown)
    with pytest.raises(ValueError, match="n_ops differs"):
        S.light_changes(sc, scenes["scene"])
    worn = sc.clone()
    root = worn.roots()[0]
    worn.c.nodes[root].material = (worn.c.nodes[root].material + 1) % worn.c.n_materials
    with pytest.raises(ValueError, match="wears material"):
        S.light_changes(sc, worn.with_lighting(points=[(0, 0, 0), None]))


# ------------------------------------------------------------------------------------------------------------------------ the CLI
def test_the_cli_refuses_what_does_not_go_with_move_lights(capsys, tmp_path):
    path = os.path.join(SCENES, "scene4.lol")
    out = str(tmp_path / "looks")
    text = "--move-lights goes with --relight"
    for extra in (["--samples", "2"], ["--lens", "0.1", "--focus", "4"], ["--adaptive", "16", "--samples", "2"],
                  ["--lens", "0.1", "--focus-at", "3,3"]):
        assert cli_main([path, "--relight", path, "--move-lights", "--size", "8x8", "-o", out] + extra) == 1, extra
        assert text in capsys.readouterr().err, extra
    assert cli_main([path, "--move-lights", "--size", "8x8"]) == 1                                # not without --relight
    assert text in capsys.readouterr().err
    # a look whose geometry differs is still refused, with its first difference, before any device is opened
    grown = open(path).read().replace("radius\t\t= 1\n", "radius\t\t= 1.25\n", 1)
    assert grown != open(path).read()
    other = str(tmp_path / "grown.lol")
    with open(other, "w") as f:
        f.write(grown)
    assert cli_main([path, "--relight", other, "--move-lights", "--size", "8x8", "-o", out]) == 1
    assert "differs in a number" in capsys.readouterr().err and not os.path.exists(out)
