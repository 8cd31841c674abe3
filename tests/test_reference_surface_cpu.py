"""Drop-in boundary check: every name the reference's run / eval scripts import from the package,
every function of ours they call and every keyword they pass must resolve against THIS package.

What the scripts use is recorded in tests/golden/reference_surface.json (names, keywords and argument counts, written
by tests/golden/make_surface.py from the reference checkout; nothing of the scripts is imported, executed or copied)."""
import dataclasses
import importlib
import inspect
import json
import os

import pytest

SURFACE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_surface.json")
with open(SURFACE_FILE) as _f:
    SURFACE = json.load(_f)
# the experiment / evaluation scripts (the callers of the surface); runs/_model.py, _helper.py and _loader.py ARE the
# surface and are replaced by this package's own files of the same names
SCRIPTS = sorted(SURFACE)


def _accepts(fn, kw):
    if dataclasses.is_dataclass(fn):
        return kw in {f.name for f in dataclasses.fields(fn)}
    try:
        sig = inspect.signature(fn)
    except (TypeError, ValueError):
        return True
    return kw in sig.parameters or any(p.kind == p.VAR_KEYWORD for p in sig.parameters.values())


@pytest.mark.parametrize("path", SCRIPTS)
def test_reference_script_resolves_against_the_package(path):
    use = SURFACE[path]
    bound = {}                                      # local name -> object of ours
    checked = 0
    for imp in use["imports"]:
        if "from" in imp:
            mod = importlib.import_module(imp["from"])
            name = imp["name"]
            if not hasattr(mod, name):              # a submodule: from future_od.datasets import nu_scenes
                try:
                    importlib.import_module(f"{imp['from']}.{name}")
                except ImportError:
                    pass
            assert hasattr(mod, name), f"{os.path.basename(path)}: {imp['from']} has no {name}"
            bound[imp["as"] or name] = getattr(mod, name)
        else:
            mod = importlib.import_module(imp["import"])
            bound[imp["as"] or imp["import"].split(".")[0]] = mod if imp["as"] else importlib.import_module(imp["import"].split(".")[0])
        checked += 1
    # attribute of an imported module / class: nu_scenes.CATEGORY_DICT, T.JointResize, transformer.MLP ...
    for base, attr in use["attributes"]:
        obj = bound[base]
        if inspect.ismodule(obj) or inspect.isclass(obj):
            assert hasattr(obj, attr), f"{os.path.basename(path)}: {base}.{attr} missing"
            checked += 1
    # keywords of calls to imported callables
    for call in use["calls"]:
        fn = bound[call["func"][0]]
        if len(call["func"]) == 2:
            fn = getattr(fn, call["func"][1], None)
        if fn is None or not callable(fn):
            continue
        for kw in call["keywords"]:
            assert _accepts(fn, kw), f"{os.path.basename(path)}: {getattr(fn, '__name__', fn)}() takes no '{kw}'"
            checked += 1
        if not dataclasses.is_dataclass(fn) and not inspect.isclass(fn):
            try:
                params = [p for p in inspect.signature(fn).parameters.values()
                          if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
                varargs = any(p.kind == p.VAR_POSITIONAL for p in inspect.signature(fn).parameters.values())
                assert varargs or call["positional"] <= len(params), f"{os.path.basename(path)}: too many positionals for {fn.__name__}"
            except (TypeError, ValueError):
                pass
    assert checked > 0 or os.path.basename(path) == "helpers.py"        # (helpers.py imports nothing of ours)


def test_trainer_surface_used_by_the_scripts():
    from future_od.trainer import Trainer
    for name in ("train", "eval", "load_checkpoint", "save_checkpoint"):
        assert hasattr(Trainer, name), name
    from future_od.datasets import nu_images, nu_scenes
    assert len(nu_scenes.CATEGORY_DICT) == 8 and nu_images.ANNOTATED_FRAME == 6
    from config import config
    assert {"visualization_path", "checkpoint_path", "nuscenes_path", "nuimages_path"} <= set(config)


def test_positional_order_of_the_loader_factories_matches_the_reference():
    from runs._loader import get_nuim_loaders, get_nusc_loaders
    for fn in (get_nusc_loaders, get_nuim_loaders):
        names = list(inspect.signature(fn).parameters)[:7]
        assert names == ["img_size", "offsets", "args", "config", "train_batch_size", "random_aug",
                         "val_annotated_frame_override"], names
