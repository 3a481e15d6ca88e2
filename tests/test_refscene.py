"""integration/lol_refscene.c: the reference's `struct scene` pointer graph → lol_scene.

The reference scene is built by the reference's own scene.c builders (driven by the independent walker of
tests/golden/make_golden.py), converted by lol_scene_from_reference(), flattened, and compared with the program the
build's own .lol reader produces from the same file.  tests/golden/ref_scene_programs.json records what that route
yields; the build's reader is held against the recording everywhere.  Where oracle/_ref/liblol_ref.so exists (built by
`make -C oracle ref` next to the reference tree) the conversion also runs live and must yield the recording again.
"""
import importlib.util
import json
import os

import pytest

from loltracer_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "liblol_ref.so")
RECORDED = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_scene_programs.json")))["programs"]


def _mk():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("name", ["scene", "scene2", "scene3", "scene4"])
def test_reference_scene_converts_to_the_same_program(name):
    mine = S.Scene.parse_file(os.path.join(ROOT, "tests", "golden", "scenes", name + ".lol"))
    want = (mine.flatten().tables(), bytes(mine.c.camera))
    assert want == (bytes.fromhex(RECORDED[name]["tables"]), bytes.fromhex(RECORDED[name]["camera"]))
    if os.path.exists(REF_SO):
        mk = _mk()
        assert mk.converted_program(mk.load_ref(), name) == want
