"""Host checks of what csrc/splat_scene.h states once for mcmc.hip, densify.hip, splat_export.hip and splat_import.hip: the two
largest argument structs against the header's text, the names the oracles restate, and the order in which the four entry points
refuse a scene - every call here returns before a launch and without reading a pointer (no GPU needed)."""
import ctypes as C
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import densify_oracle as DO  # noqa: E402
import mcmc_oracle as MO  # noqa: E402
from c_layout import assert_mirrors  # noqa: E402

OK, ARG, SHAPE, WORKSPACE = 0, -1, -2, -4
GROUPS = ("", "m_", "v_")


@pytest.mark.parametrize("struct,name", [("McmcRelocateArgs", "v3a_mcmc_relocate_args"), ("DensifyApplyArgs", "v3a_densify_apply_args")])
def test_ctypes_struct_matches_the_header(struct, name):
    from vist3a_amd import lib
    assert_mirrors(getattr(lib, struct), name)


def test_the_oracles_name_the_tensors_as_the_library_does():
    from vist3a_amd import lib, ops
    assert MO.NAMES == DO.NAMES == ops.SPLAT_TENSORS and len(lib.SPLAT_FIELDS) == len(ops.SPLAT_TENSORS)


def _min_ld(K):
    return dict(ld_means=3, ld_log_scales=3, ld_quats=4, ld_logits=1, ld_sh=3 * (K + 1))


def _strided(a, K):
    from vist3a_amd import lib
    for f in lib.SPLAT_FIELDS:
        setattr(a, f, 256)
    for f, ld in _min_ld(K).items():
        setattr(a, f, ld)


@pytest.mark.parametrize("K", [0, 1])
def test_export_refusal_order(K):
    from vist3a_amd import lib
    L = lib.load()
    rest = (L.v3a_splat_export_sort, L.v3a_splat_export_pack_compressed, L.v3a_splat_export_pack_splat, L.v3a_splat_export_pack_ply)
    a = lib.SplatExportArgs()
    a.K = K
    assert all(f(C.byref(a), None) == OK for f in rest)                    # U = 0, n = 0, every pointer null: nothing to do
    assert L.v3a_splat_export_filter(C.byref(a), None) == ARG              # ... but the filter still owes the count
    a.K = 1025
    assert L.v3a_splat_export_filter(C.byref(a), None) == SHAPE            # the K limit comes before the empty scene
    a.U, a.K = 4, K
    _strided(a, K)
    assert L.v3a_splat_export_filter(C.byref(a), None) == ARG              # the scene passes; count is null
    for f in lib.SPLAT_FIELDS:
        setattr(a, f, None)
        a.ld_quats = 3
        assert L.v3a_splat_export_filter(C.byref(a), None) == ARG, f       # a null tensor is reported before a short stride
        a.ld_quats = 4
        assert all(g(C.byref(a), None) == ARG for g in rest), f
        setattr(a, f, 256)
    for f, ld in _min_ld(K).items():
        setattr(a, f, ld - 1)
        assert L.v3a_splat_export_filter(C.byref(a), None) == SHAPE, f
        assert all(g(C.byref(a), None) == SHAPE for g in rest), f
        setattr(a, f, ld)
    a.U = -1
    assert L.v3a_splat_export_filter(C.byref(a), None) == SHAPE


@pytest.mark.parametrize("K", [0, 1])
def test_import_refusal_order(K):
    from vist3a_amd import lib
    L = lib.load()
    n = 4
    a = lib.SplatImportArgs()
    a.n_rest = 3 * K
    if K == 0:
        call, a.payload_bytes = L.v3a_splat_import_splat, 32 * n
    else:
        call, a.nch, a.payload_bytes = L.v3a_splat_import_compressed, 1, 72 + 16 * n + 3 * K * n
    assert call(None, None) == ARG and call(C.byref(a), None) == OK        # n = 0, every pointer null: nothing to do
    a.n = n
    _strided(a, K)
    a.bad = a.payload = 256
    assert call(C.byref(a), None) == WORKSPACE                             # everything about the scene passes; no workspace
    for f in lib.SPLAT_FIELDS + ("bad", "payload"):
        setattr(a, f, None)
        a.ld_quats = 3
        assert call(C.byref(a), None) == ARG, f                            # a null pointer is reported before a short stride
        a.ld_quats = 4
        setattr(a, f, 256)
    for f, ld in _min_ld(K).items():
        setattr(a, f, ld - 1)
        assert call(C.byref(a), None) == SHAPE, f
        setattr(a, f, ld)
    a.payload = 258
    assert call(C.byref(a), None) == SHAPE                                 # the payload's alignment


def test_mcmc_relocate_refusal_order():
    from vist3a_amd import lib
    L = lib.load()
    a = lib.McmcRelocateArgs()
    assert L.v3a_mcmc_relocate(C.byref(a), None) == ARG                    # U = 0 is not a no-op here: null pointers come first
    pointers = ["src", "counts"] + [g + f for g in GROUPS for f in lib.SPLAT_FIELDS]
    assert pointers == [f for f, _ in lib.McmcRelocateArgs._fields_[:17]]
    for f in pointers:
        setattr(a, f, 8)
    assert L.v3a_mcmc_relocate(C.byref(a), None) == SHAPE                  # U = 0
    a.U, a.n_slots, a.K, a.min_opacity = 4, 4, 1, 0.005                    # all but the workspace: the call below stops at -4
    assert L.v3a_mcmc_relocate(C.byref(a), None) == WORKSPACE
    for f in pointers:
        setattr(a, f, None)
        assert L.v3a_mcmc_relocate(C.byref(a), None) == ARG, f
        a.K = 0
        assert L.v3a_mcmc_relocate(C.byref(a), None) == ARG, f            # before the shape
        a.K = 1
        setattr(a, f, 8)


def test_densify_apply_refusal_order():
    from vist3a_amd import lib
    L = lib.load()
    b = lib.DensifyApplyArgs()
    b.K = 4
    assert L.v3a_densify_apply(C.byref(b), None) == OK                     # U = U_out = 0, every pointer null: nothing to do
    b.U = 100
    assert L.v3a_densify_apply(C.byref(b), None) == OK                     # U_out = 0
    b.U_out = 150
    assert L.v3a_densify_apply(C.byref(b), None) == ARG
    tensors = [g + f for g in GROUPS + tuple("new_" + g for g in GROUPS) for f in lib.SPLAT_FIELDS]
    assert tensors == [f for f, _ in lib.DensifyApplyArgs._fields_[:30]]
    for i, f in enumerate(tensors):
        setattr(b, f, (i + 1) << 20)                                       # 1 MiB apart: no two tensors overlap
    b.fates = b.offsets = 8                                                # totals stays null: no call here goes past the checks
    for f in tensors:
        keep = getattr(b, f)
        setattr(b, f, None)
        b.totals = 8
        assert L.v3a_densify_apply(C.byref(b), None) == ARG, f
        b.totals = None
        setattr(b, f, keep)
    b.new_sh = b.sh
    assert L.v3a_densify_apply(C.byref(b), None) == ARG                    # a null pointer is reported before an overlap
