"""The host package is layered: module-level imports inside kimimaro_amd only go downward in ORDER, nothing but Engine.soma_lane_pool
imports a sibling inside a function, and what left intake.py or post.py for a module of its own is still reachable there.  No GPU, no library:
the import graph is read from the source with ast."""
import ast
import importlib
import os

import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kimimaro_amd")

# low to high: a module imports, at module level, only modules in front of it
ORDER = ("_abi", "skeleton", "build", "plan", "volume", "holes", "border", "assemble", "engine", "feature", "points", "section",
         "ops", "trace", "avocado", "intake", "utility", "lanes", "distributed", "boxes", "region_boxes", "section_boxes", "segment_boxes",
         "point_boxes", "post")

# name -> the module that defines it; each is the same object as kimimaro_amd.intake.NAME
LEGACY = {
    "LazyVolume": "volume", "format_labels": "volume", "apply_object_mask": "volume", "DimensionError": "volume",
    "Assembler": "assemble", "assemble": "assemble", "paths_of": "assemble", "consolidate_paths": "assemble",
    "consolidate_paths_flat": "assemble", "consolidate_paths_flat_numpy": "assemble", "consolidate_paths_batch": "assemble",
    "resolve_holes": "holes", "enclosed_regions": "holes",
    "_avocado_fruit_from_lines": "avocado", "engage_avocado_protection_device": "avocado",
    "TRACE_DEFAULTS": "trace",
    "skeletonize": "intake", "skeletonize_cc": "intake", "shard_components": "intake", "compute_cc_labels": "intake",
    "compute_cc_labels_device": "intake", "fill_all_holes": "intake", "fill_all_holes_device": "intake",
    "synapses_to_targets": "intake", "connect_points": "intake", "DEFAULT_TEASAR_PARAMS": "intake",
}

# name -> the module that defines it; each is the same object as kimimaro_amd.post.NAME
POST = {
    "region_graph_chunked": "region_boxes", "hole_lists": "region_boxes", "RegionGraph": "region_boxes", "_merge_regions": "region_boxes",
    "fill_all_holes_chunked": "region_boxes",
    "synapses_to_targets_chunked": "point_boxes",
    "route_targets": "boxes", "count_labels": "boxes",
    "cross_sectional_area_chunked": "section_boxes", "cross_sectional_area_filled_chunked": "section_boxes", "XS_CLIPPED": "section_boxes",
    "oversegment_chunked": "segment_boxes", "shell_diff": "segment_boxes", "DIRECTIONS": "segment_boxes",
}


def _modules():
    return sorted(f[:-3] for f in os.listdir(PKG) if f.endswith(".py") and f != "__init__.py")


def _siblings(node, known):
    """the modules of the package an Import / ImportFrom node names"""
    if isinstance(node, ast.ImportFrom) and node.level == 1:
        if node.module is None:                                    # from . import a, b
            return [a.name for a in node.names if a.name in known]
        return [node.module.split(".")[0]]                         # from .a import x
    names = [node.module] if isinstance(node, ast.ImportFrom) and node.level == 0 else \
        [a.name for a in node.names] if isinstance(node, ast.Import) else []
    return [n.split(".")[1] for n in names if n and n.startswith("kimimaro_amd.")]


def _edges(module, known):
    """(module-level, function-level) sets of sibling modules `module` imports"""
    with open(os.path.join(PKG, module + ".py")) as f:
        tree = ast.parse(f.read())
    top, inner = set(), set()

    def walk(node, inside):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, (ast.Import, ast.ImportFrom)):
                (inner if inside else top).update(_siblings(child, known))
            walk(child, inside or isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)))

    walk(tree, False)
    return top, inner


def test_every_module_has_a_layer():
    assert sorted(ORDER) == _modules()


@pytest.mark.parametrize("module", ORDER)
def test_module_level_imports_go_downward(module):
    top, _ = _edges(module, set(ORDER))
    upward = sorted(m for m in top if m not in ORDER or ORDER.index(m) >= ORDER.index(module))
    assert not upward, "%s imports %s at module level: not below it in the layering" % (module, upward)


def test_only_the_soma_lane_pool_imports_inside_a_function():
    found = {(m, s) for m in ORDER for s in _edges(m, set(ORDER))[1]}
    assert found == {("engine", "lanes")}


@pytest.mark.parametrize("name", sorted(LEGACY))
def test_legacy_name_is_the_same_object(name):
    intake = importlib.import_module("kimimaro_amd.intake")
    home = importlib.import_module("kimimaro_amd." + LEGACY[name])
    assert hasattr(intake, name), "kimimaro_amd.intake.%s is gone" % name
    assert getattr(intake, name) is getattr(home, name)
    assert getattr(getattr(home, name), "__module__", home.__name__) == home.__name__     # defined there, not passed through


@pytest.mark.parametrize("name", sorted(POST))
def test_post_name_is_the_same_object(name):
    post = importlib.import_module("kimimaro_amd.post")
    home = importlib.import_module("kimimaro_amd." + POST[name])
    assert hasattr(post, name), "kimimaro_amd.post.%s is gone" % name
    assert getattr(post, name) is getattr(home, name)
    assert getattr(getattr(home, name), "__module__", home.__name__) == home.__name__     # defined there, not passed through
