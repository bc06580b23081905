"""The layout of a struct of include/vist3a_hip.h as the C compiler lays it out (LP64), read from the header's text: what the
ctypes mirrors of vist3a_amd/lib.py are held to."""
import ctypes as C
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
_SIZES = {"char": 1, "int": 4, "float": 4, "long": 8, "long long": 8, "double": 8}


def header_text() -> str:
    """include/vist3a_hip.h without its comments"""
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "vist3a_hip.h").read_text(), flags=re.S)


def _layout(txt: str, name: str):
    """({field: (offset, size)}, size, alignment) of the typedef struct `name`"""
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", txt).group(1)
    off, fields, biggest = 0, {}, 1
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        first, *more = [p.strip() for p in decl.split(",")]
        base = first[:re.search(r"[\w\[\]]+$", first).start()].strip()            # the type in front of the first declarator
        scalar = base.replace("const", "").replace("unsigned", "").strip() or "int"
        for d in [first[len(base):].strip()] + more:
            pointer = d.startswith("*") or base.endswith("*")
            m = re.fullmatch(r"\*?\s*(\w+)(?:\[(\d+)\])?", d)
            if pointer:
                size = align = 8
            elif scalar in _SIZES:
                size = align = _SIZES[scalar]
            else:                                                                 # an earlier typedef struct of the header, embedded
                _, size, align = _layout(txt, scalar)
            count = int(m.group(2) or 1)
            off = (off + align - 1) // align * align
            fields[m.group(1)] = (off, size * count)
            off += size * count
            biggest = max(biggest, align)
    return fields, (off + biggest - 1) // biggest * biggest, biggest


def c_layout(name: str):
    """{field: (offset, size)} and the total size of the typedef struct `name` (pointers and longs 8 bytes, ints 4, natural
    alignment; a field whose type is another struct of the header has that struct's size and alignment)"""
    fields, size, _ = _layout(header_text(), name)
    return fields, size


def assert_mirrors(struct, name: str) -> None:
    """the ctypes Structure `struct` has the fields of the header's `name` in order, each at its offset with its size, and its sizeof"""
    fields, size = c_layout(name)
    assert [f for f, _ in struct._fields_] == list(fields)
    for f, (off, sz) in fields.items():
        d = getattr(struct, f)
        assert (d.offset, d.size) == (off, sz), (f, d.offset, d.size, off, sz)
    assert C.sizeof(struct) == size
