"""Host checks of the scene import: the header parser of vist3a_amd/utils/splat_import.py (property orders, skipped properties,
every refusal), the fp32 twin of tests/splat_import_oracle.py against the fp64 decoders of tests/splat_export_oracle.py on every
fixture file, the ctypes struct against the header's declaration, and the C ABI's refusals (no GPU needed)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import splat_export_oracle as SO  # noqa: E402
import splat_import_oracle as IO  # noqa: E402
from c_layout import assert_mirrors  # noqa: E402

CASES = tuple(SO.CASES)


@pytest.fixture(scope="module")
def fx():
    return SO.load_fixture()


def _bytes(fx, case, fmt):
    return fx[f"{case}.{fmt}"].numpy().tobytes()


# --------------------------------------------------------------------------------------------------------------------- parser
@pytest.mark.parametrize("case", CASES)
def test_parser_reads_the_fixture_files(fx, case):
    from vist3a_amd import ops
    from vist3a_amd.utils.splat_import import parse_header
    N, K = SO.CASES[case]
    for fmt in SO.FORMATS:
        data = _bytes(fx, case, fmt)
        got_fmt, n, k, table, off = parse_header(data)
        assert got_fmt == fmt
        if fmt == "splat":
            assert (n, k, table, off) == (len(data) // 32, 0, {}, 0)
            continue
        head, body = SO.split_header(data)
        assert off == len(head) and k == K and n <= N
        if fmt == "ply":
            names = IO.ply_names(data)
            assert table["P"] == 14 + 3 * K and all(table[p] == names.index(p) for p in ops.PLY_COLUMNS if p in names)
            assert len(body) == 4 * n * table["P"]
        else:
            assert n == SO.parse_compressed(data)["n"] and table == {}


def test_parser_takes_any_property_order_and_skips_extras(fx):
    from vist3a_amd.utils.splat_import import parse_header
    data = _bytes(fx, "B", "ply")                                  # K = 3: P = 23, f_rest_0..8 at 6..14
    P = 23
    blocks = [list(range(15, 23)), list(range(6, 15)), [3, 4, 5], [2, 0, 1]]      # tail first, the f_rest run kept together
    order = [i for b in blocks for i in b]
    assert sorted(order) == list(range(P))
    moved = IO.permute_ply(data, order, extra=("nx", "ny", "nz"))
    fmt, n, K, table, off = parse_header(moved)
    names = IO.ply_names(moved)
    assert (fmt, n, K) == ("ply", 257, 3) and table["P"] == P + 3 and names[:3] == ["nx", "ny", "nz"]
    for p in IO.PLY_NAMES + ("f_rest_0",):
        assert table[p] == names.index(p), p
    assert table["x"] == 3 + order.index(0) and table["f_rest_0"] == 3 + 8
    a, b = IO.twin_ply(moved), IO.twin_ply(data)                   # the same scene
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_parser_refusals(fx):
    from vist3a_amd.utils.splat_import import parse_header
    data = _bytes(fx, "E", "ply")                                  # one splat, K = 2
    head, body = SO.split_header(data)
    names = IO.ply_names(data)
    with pytest.raises(ValueError, match="binary_little_endian"):
        parse_header(IO.ply_header(1, names, fmt="binary_big_endian") + body)
    with pytest.raises(ValueError, match="binary_little_endian"):
        parse_header(IO.ply_header(1, names, fmt="ascii") + body)
    types = ["float"] * len(names)
    types[names.index("opacity")] = "uchar"
    with pytest.raises(ValueError, match="non-float vertex property `uchar opacity`"):
        parse_header(IO.ply_header(1, names, types) + body)
    for gone in ("x", "f_dc_2", "opacity", "scale_1", "rot_3"):
        keep = [p for p in names if p != gone]
        with pytest.raises(ValueError, match=f"missing property `{gone}`"):
            parse_header(IO.ply_header(1, keep) + body[:4 * len(keep)])
    with pytest.raises(ValueError, match="f_rest"):                # 5 harmonics columns: not a multiple of 3
        parse_header(IO.ply_header(1, [p for p in names if p != "f_rest_5"]) + body[:-4])
    with pytest.raises(ValueError, match="truncated"):
        parse_header(data[:-1])
    with pytest.raises(ValueError, match="over-long"):
        parse_header(data + b"\0")
    with pytest.raises(ValueError, match="list properties"):
        parse_header(head.replace(b"end_header\n", b"element face 0\nproperty list uchar int vertex_indices\nend_header\n") + body)
    comp = _bytes(fx, "B", "ply_compressed")                       # 2 chunks
    with pytest.raises(ValueError, match="chunk count must be"):
        parse_header(comp.replace(b"element chunk 2\n", b"element chunk 3\n"))
    with pytest.raises(ValueError, match="truncated"):
        parse_header(comp[:-1])
    with pytest.raises(ValueError, match="over-long"):
        parse_header(comp + b"\0")
    with pytest.raises(ValueError, match="missing property"):
        parse_header(comp.replace(b"property uint packed_scale\n", b""))
    with pytest.raises(ValueError, match="multiple of 32"):
        parse_header(b"\0" * 33)


def test_parser_empty_files():
    from vist3a_amd.utils.splat_import import parse_header
    assert parse_header(b"") == ("splat", 0, 0, {}, 0)
    assert parse_header(b"\1" * 32) == ("splat", 1, 0, {}, 0)
    head = SO.header_ply(0, 2)
    fmt, n, K, table, off = parse_header(head)
    assert (fmt, n, K, off, table["P"]) == ("ply", 0, 2, len(head), 20)
    head = SO.header_compressed(0, 1)
    assert parse_header(head) == ("ply_compressed", 0, 1, {}, len(head))
    fmt, n, K, table, off = parse_header(SO.header_ply(0, 0))
    assert K == 0 and table["f_rest_0"] == 0


# ------------------------------------------------------------------------------------------------------- the twin against fp64
@pytest.mark.parametrize("case", CASES)
def test_twin_is_within_the_bounds_of_the_fp64_decode(fx, case):
    data = _bytes(fx, case, "ply_compressed")
    t, r = IO.twin_compressed(data), IO.ref_compressed(data)
    n = t["means"].shape[0]
    b = np.repeat(r["chunks"].astype(np.float64), 256, axis=0)[:n]
    err = lambda k: np.abs(t[k].astype(np.float64) - r[k])
    assert (err("means") <= IO.lerp_bound(b[:, 0:3], b[:, 3:6])).all()
    assert (err("scales") <= IO.lerp_bound(b[:, 6:9], b[:, 9:12])).all()
    rgb = r["sh"][:, :, 0] * SO.C0 + 0.5
    assert (err("sh")[:, :, 0] <= IO.sh0_bound(IO.lerp_bound(b[:, 12:15], b[:, 15:18]), rgb)).all()
    assert np.array_equal(t["sh"][:, :, 1:].astype(np.float64), r["sh"][:, :, 1:])          # exact in fp32
    assert (err("opacities") <= IO.log_bound(r["opacities"])).all()
    stored = np.arange(4)[None, :] != r["rot_index"][:, None]
    assert (err("quats")[stored] <= IO.ROT_BOUND).all() and (err("quats")[~stored] <= IO.DROPPED_BOUND).all()
    data = _bytes(fx, case, "splat")
    t, r = IO.twin_splat(data), IO.ref_splat(data)
    err = lambda k: np.abs(t[k].astype(np.float64) - r[k])
    assert np.array_equal(t["means"].astype(np.float64), r["means"]) and np.array_equal(t["quats"].astype(np.float64), r["quats"])
    assert (err("scales") <= IO.log_bound(r["scales"])).all() and (err("opacities") <= IO.log_bound(r["opacities"])).all()
    rgb = r["sh"][:, :, 0] * SO.C0 + 0.5
    assert (err("sh")[:, :, 0] <= IO.sh0_bound(2 * IO.EPS * rgb, rgb)).all()
    print(f"[splat import twin] {case}: max logit err {err('opacities').max():.3g}, max log-scale err {err('scales').max():.3g}")


@pytest.mark.parametrize("case", CASES)
def test_twin_ply_equals_the_fixture_inputs(fx, case):
    x = SO.fixture_inputs(fx, case)
    rows = SO.valid_rows(**x)
    t = IO.twin_ply(_bytes(fx, case, "ply"))
    sh = torch.cat([x["sh0"], x["shN"]], dim=1).permute(0, 2, 1).contiguous()
    want = dict(means=x["means"], scales=x["scales"], quats=x["quats"], opacities=x["opacities"], sh=sh)
    for k, v in want.items():
        assert t[k].tobytes() == v[rows].contiguous().numpy().tobytes(), k


def test_linear_opacity_twin():
    o = np.array([0.0, 1e-7, 0.25, 0.5, 1.0, 2.0, np.nan], dtype=np.float32)
    got = IO.logit_linear32(o)
    assert np.isnan(got[-1]) and np.isfinite(got[:-1]).all()
    assert (np.abs(got[:-1] - IO.logit_linear64(o[:-1])) <= IO.log_bound(IO.logit_linear64(o[:-1]))).all()
    assert got[3] == 0 and got[0] == got[1] and got[4] == got[5]                   # clamped at both ends


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_ctypes_struct_matches_the_header():
    from vist3a_amd import lib
    assert_mirrors(lib.SplatImportArgs, "v3a_splat_import_args")                  # names in order, every (offset, size), sizeof
    assert_mirrors(lib.SplatExportArgs, "v3a_splat_export_args")
    assert lib.EXPECTED_ABI >= 35


def test_c_abi_refuses_bad_arguments():
    """the entry points return their error codes before any launch and without reading a pointer (safe without a GPU)"""
    from vist3a_amd import lib
    L = lib.load()
    entry = (L.v3a_splat_import_ply, L.v3a_splat_import_compressed, L.v3a_splat_import_splat)
    assert L.v3a_splat_import_workspace_bytes(-1) == -2 and L.v3a_splat_import_workspace_bytes(1 << 31) == -2
    assert L.v3a_splat_import_workspace_bytes(257) == 256 and L.v3a_splat_import_workspace_bytes(0) == 0
    for f in entry:
        assert f(None, None) == -1
    a = lib.SplatImportArgs()
    for f in entry:
        assert f(C.byref(a), None) == 0                                            # n = 0: nothing to do, nothing looked at
    a.n = -1
    for f in entry:
        assert f(C.byref(a), None) == -2
    a.n = 300
    for f in entry:
        assert f(C.byref(a), None) == -1                                           # null pointers
    a.means = a.log_scales = a.quats = a.logits = a.sh = a.bad = a.payload = a.workspace = 256
    a.workspace_bytes = 256
    a.ld_means = a.ld_log_scales = 3
    a.ld_quats, a.ld_logits, a.ld_sh = 4, 1, 3
    for bad_rest in (-3, 4, 192):                                                  # negative, not a multiple of 3, K = 64
        a.n_rest = bad_rest
        for f in entry:
            assert f(C.byref(a), None) == -2, bad_rest
    a.n_rest = 6
    for f in entry:
        assert f(C.byref(a), None) == -2                                           # sh rows overlap: 3 (K + 1) = 9
    a.ld_sh = 9
    # float PLY: K = 2, P = 20
    cols = list(range(20))
    order = cols[:6] + [6] + cols[12:]                                             # x y z dc rest@6 opacity scale rot
    def ply(P=20, offsets=order, payload_bytes=4 * 300 * 20, payload=256, ws_bytes=512):
        a.P, a.payload_bytes, a.payload, a.workspace_bytes = P, payload_bytes, payload, ws_bytes
        for j, o in enumerate(offsets):
            a.offsets[j] = o
        return L.v3a_splat_import_ply(C.byref(a), None)
    assert ply(offsets=order[:14] + [20]) == -2                                    # an offset >= P
    assert ply(offsets=order[:6] + [15] + order[7:]) == -2                         # the f_rest run passes the row's end
    assert ply(offsets=[1] + order[1:]) == -2                                      # x and y in one column
    assert ply(offsets=order[:7] + [7] + order[8:]) == -2                          # opacity inside the f_rest run
    assert ply(P=19) == -2 and ply(P=4097, payload_bytes=4 * 300 * 4097) == -2
    assert ply(payload_bytes=4 * 300 * 20 - 1) == -2 and ply(payload_bytes=4 * 300 * 20 + 4) == -2
    assert ply(payload=258) == -2                                                  # payload not 4-byte aligned
    assert ply(ws_bytes=255) == -4
    # compressed: 2 chunks, K = 2
    def comp(nch=2, payload_bytes=72 * 2 + 22 * 300, ws_bytes=512):
        a.nch, a.payload_bytes, a.workspace_bytes = nch, payload_bytes, ws_bytes
        return L.v3a_splat_import_compressed(C.byref(a), None)
    assert comp(nch=1, payload_bytes=72 + 22 * 300) == -2 and comp(nch=3, payload_bytes=72 * 3 + 22 * 300) == -2
    assert comp(payload_bytes=72 * 2 + 22 * 300 - 1) == -2 and comp(ws_bytes=8) == -4
    # .splat
    a.payload_bytes, a.workspace_bytes = 32 * 300, 512
    assert L.v3a_splat_import_splat(C.byref(a), None) == -2                        # harmonics in a .splat
    a.n_rest, a.ld_sh, a.payload_bytes = 0, 3, 32 * 300 - 1
    assert L.v3a_splat_import_splat(C.byref(a), None) == -2
    a.payload_bytes, a.workspace_bytes = 32 * 300, 0
    assert L.v3a_splat_import_splat(C.byref(a), None) == -4


def test_wrappers_refuse_host_tensors():
    from vist3a_amd import ops
    with pytest.raises(ValueError, match="device vector"):
        ops.splat_import_splat(torch.zeros(32, dtype=torch.uint8), 1)
    with pytest.raises(ValueError, match="opacity must be"):
        ops.splat_import_ply(torch.zeros(56, dtype=torch.uint8), 1, 0, {}, opacity="alpha")
