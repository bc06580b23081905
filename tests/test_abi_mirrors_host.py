"""Every ctypes mirror of vist3a_amd/lib.py against the text of include/vist3a_hip.h: each argument struct's layout, and each
prototype's return and parameter types.  Nothing is compiled and no library is loaded."""
import ctypes as C
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from c_layout import assert_mirrors, header_text  # noqa: E402

from vist3a_amd import lib  # noqa: E402

_PROTO = re.compile(r"((?:const\s+)?(?:unsigned\s+)?(?:long\s+long|\w+)\s*\**)\s*\b(v3a_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")
_SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
            "uint32_t": C.c_uint32, "unsigned int": C.c_uint32, "uint64_t": C.c_uint64, "unsigned long long": C.c_uint64}


def _prototypes():
    """{name: (return type, [parameter types])} of every prototype of the header, the types as written (names and spacing removed)"""
    out = {}
    for ret, name, params in _PROTO.findall(header_text()):
        params = [" ".join(p.split()) for p in params.split(",")]
        types = [] if params == ["void"] else [re.sub(r"\s*\b\w+$", "", p).replace(" *", "*") for p in params]   # every parameter is named
        assert name not in out and all(types), name
        out[name] = (" ".join(ret.split()).replace(" *", "*"), types)
    return out


def _struct_typedefs():
    return re.findall(r"typedef struct \{[^}]*\}\s*(v3a_\w+_args)\s*;", header_text())


def _mirror_of():
    """{header struct: its ctypes class}, found through the entry points that take `const v3a_X_args*` first"""
    found = {}
    for name, (_, params) in _prototypes().items():
        m = re.fullmatch(r"const (v3a_\w+_args)\*", params[0]) if params else None
        if m:
            cls = lib.SYMBOLS[name][1][0]._type_
            assert found.setdefault(m.group(1), cls) is cls, f"{m.group(1)} is mirrored by two classes ({name})"
    return found


def test_parser_sees_every_declaration():
    declared = sorted(set(re.findall(r"\b(v3a_[a-z0-9_]+)\s*\(", header_text())))
    assert sorted(_prototypes()) == declared == sorted(lib.SYMBOLS)


def test_every_struct_mirrors_its_typedef():
    typedefs, mirrors = _struct_typedefs(), _mirror_of()
    classes = [v for v in vars(lib).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure]
    assert sorted(mirrors) == sorted(typedefs), "a struct of the header that no entry point takes, or the reverse"
    assert len(set(mirrors.values())) == len(mirrors) == len(classes) and set(mirrors.values()) == set(classes), \
        "the header's structs and lib.py's Structure subclasses are not in one-to-one correspondence"
    for name in typedefs:
        assert_mirrors(mirrors[name], name)


def _is_pointer(t) -> bool:
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def _matches(c_type: str, ct, mirrors) -> bool:
    if c_type in _SCALARS:
        return ct is _SCALARS[c_type]
    m = re.fullmatch(r"const (v3a_\w+_args)\*", c_type)
    if m:
        return ct is C.POINTER(mirrors[m.group(1)])
    return c_type.endswith("*") and _is_pointer(ct)


def test_every_prototype_matches_its_binding():
    mirrors = _mirror_of()
    wrong = []
    for name, (ret, params) in _prototypes().items():
        res, args = lib.SYMBOLS[name]
        if len(args) != len(params):
            wrong.append((name, "argument count", len(params), len(args)))
            continue
        if not _matches(ret, res, mirrors):
            wrong.append((name, "return", ret, res))
        wrong += [(name, i, p, a) for i, (p, a) in enumerate(zip(params, args)) if not _matches(p, a, mirrors)]
    assert not wrong, wrong
