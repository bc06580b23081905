"""vist3a_amd.ops is one namespace over several modules: every `ops.X` the code base writes resolves, the hot path and the state
other code rebinds are defined in ops itself, and importing it needs neither a GPU nor the shared library."""
import ast
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def _sources():
    for top in ("vist3a_amd", "tests", "tools", "evaluation"):
        yield from sorted((ROOT / top).rglob("*.py"))
    yield from (ROOT / "bench.py", ROOT / "inference_t23d.py")


def _ops_attributes(tree) -> set:
    """every X of `A.X` where the name A is bound to vist3a_amd.ops by an import somewhere in the file"""
    bound = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):          # from vist3a_amd import ops / from .. import ops [as A]: the package has one module of that name
            if node.module == "vist3a_amd" or (node.level > 0 and node.module is None):
                bound |= {a.asname or a.name for a in node.names if a.name == "ops"}
        elif isinstance(node, ast.Import):            # import vist3a_amd.ops as A
            bound |= {a.asname for a in node.names if a.name == "vist3a_amd.ops" and a.asname}
    return {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id in bound}


def test_every_ops_attribute_in_the_code_base_resolves():
    from vist3a_amd import ops
    used = {}
    for path in _sources():
        for attr in _ops_attributes(ast.parse(path.read_text(), filename=str(path))):
            used.setdefault(attr, path.relative_to(ROOT))
    assert {"gemm", "gs_render", "_ptr", "_stream", "_splat_inner", "L"} <= set(used)   # the walk finds what it should
    missing = {a: str(p) for a, p in used.items() if not hasattr(ops, a)}
    assert not missing, missing


def test_hot_path_and_state_are_defined_in_ops_itself():
    from vist3a_amd import ops
    for name in ("gemm", "_gemm_skinny", "set_gemm_probe", "set_flop_meter"):
        assert getattr(ops, name).__module__ == "vist3a_amd.ops", name
    for name in ("_probe", "_meter", "_gemm_ws", "_attn_ws"):
        assert name in vars(ops), name
    # the setters rebind the globals that wan/dit.py and t23d.py read through `ops`
    meter = ops.FlopMeter()
    ops.set_flop_meter(meter)
    try:
        assert ops._meter is meter
    finally:
        ops.set_flop_meter(None)
    assert ops._meter is None


def test_the_torch_global_is_swapped_in_every_wrapper_module():
    """tests/test_guard_bands_gpu.py assigns `ops.torch`: the wrappers of the _ops modules must allocate through it as well"""
    import torch
    from vist3a_amd import _ops, ops
    modules = [getattr(_ops, m) for m in ("common", "raster", "metrics", "post_opt", "scene")]
    stand_in = object()
    ops.torch = stand_in
    try:
        assert all(m.torch is stand_in for m in modules) and vars(ops)["torch"] is stand_in
    finally:
        ops.torch = torch
    assert all(m.torch is torch for m in modules) and ops.torch is torch


def test_importing_ops_loads_no_library_and_needs_no_gpu():
    code = ("import vist3a_amd.ops as ops, vist3a_amd.lib as lib, torch; assert lib._lib is None; "
            "assert not torch.cuda.is_initialized(); assert callable(ops.gemm) and callable(ops.gs_render)")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
