"""mergenet_amd/abi.py against include/mergenet_hip.h, parameter by parameter (no library, no GPU).

A c_int where the header has `long long`, or a dropped argument, reaches a kernel launch as a wrong pointer, and
nothing on the host would notice.  So every prototype of the header is reduced to kinds -- pointer, i32, i64, f32, f64,
size_t, void -- and compared with ``abi.SIGNATURES``; every integer ``MN_*`` of abi.py with the header's #define or
enumerator; the members of ``mn_options`` and ``mn_stats`` with the ctypes structures' fields."""
import ctypes
import os
import re

from mergenet_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the header says these three in prose (mn_options.require_proof: 1 / 0 / -1), not as names
PYTHON_ONLY = {"MN_PROVE_ALWAYS": 1, "MN_PROVE_BY_MODE": 0, "MN_PROVE_NEVER": -1}


def header_text() -> str:
    text = open(os.path.join(ROOT, "include", "mergenet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def c_kind(decl: str) -> str:
    """The kind of a C return type, parameter or member, its name (if any) still attached."""
    if "*" in decl:
        return "pointer"
    words = [w for w in re.findall(r"[A-Za-z_][A-Za-z0-9_]*", decl) if w != "const"]
    for kind, spelling in (("i64", ["long", "long"]), ("size_t", ["size_t"]), ("f32", ["float"]), ("f64", ["double"]),
                           ("i32", ["int"]), ("i32", ["unsigned"]), ("void", ["void"])):
        if words[:len(spelling)] == spelling and len(words) <= len(spelling) + 1:
            return kind
    raise AssertionError("a C type this test does not know: %r" % decl)


def ctypes_kind(t) -> str:
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or isinstance(t, type(ctypes.POINTER(ctypes.c_int))):
        return "pointer"
    return {ctypes.c_int: "i32", ctypes.c_longlong: "i64", ctypes.c_float: "f32", ctypes.c_double: "f64",
            ctypes.c_size_t: "size_t"}[t]


def header_prototypes() -> dict:
    """name -> (return kind, [parameter kinds]) of every mn_* / c_run_segmentation prototype."""
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \t]*?[ \t*]+\**)\b(mn_[a-z0-9_]+|c_run_segmentation)\s*"
                                        r"\(([^()]*)\)\s*;", header_text()):
        params = params.strip()
        kinds = [] if params in ("", "void") else [c_kind(p) for p in params.split(",")]
        assert name not in protos, "declared twice: %s" % name
        protos[name] = (c_kind(ret), kinds)
    return protos


def header_constants() -> dict:
    text = header_text()
    number = r"(-?(?:0[xX][0-9a-fA-F]+|\d+))"
    found = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MN_[A-Z0-9_]+)[ \t]+" + number + r"[ \t]*$", text, re.M):
        found[name] = int(value, 0)
    for body in re.findall(r"\benum\s+\w+\s*\{([^}]*)\}", text):
        for name, value in re.findall(r"\b(MN_[A-Z0-9_]+)\s*=\s*" + number + r"\s*(?:,|$)", body.strip()):
            found[name] = int(value, 0)
    return found


def header_struct(name: str) -> list:
    """[(member, kind)] of `typedef struct NAME { ... } NAME;`, in order."""
    m = re.search(r"typedef\s+struct\s+%s\s*\{([^}]*)\}\s*%s\s*;" % (name, name), header_text())
    assert m, "include/mergenet_hip.h has no typedef struct %s" % name
    members = []
    for decl in m.group(1).split(";"):
        if decl.strip():
            members.append((re.findall(r"[A-Za-z_][A-Za-z0-9_]*", decl)[-1], c_kind(decl)))
    return members


def test_every_prototype_is_bound_and_nothing_else():
    protos = header_prototypes()
    assert len(protos) >= 51, "the parser found only %d prototypes" % len(protos)
    assert set(protos) == set(abi.SIGNATURES), sorted(set(protos) ^ set(abi.SIGNATURES))
    assert abi.EXPORTS == list(abi.SIGNATURES)


def test_every_signature_agrees_with_its_prototype():
    wrong = []
    for name, (ret, params) in sorted(header_prototypes().items()):
        restype, argtypes = abi.SIGNATURES[name]
        bound = [ctypes_kind(t) for t in argtypes]
        if ctypes_kind(restype) != ret:
            wrong.append("%s returns %s, bound as %s" % (name, ret, ctypes_kind(restype)))
        if len(bound) != len(params):
            wrong.append("%s takes %d parameters, bound with %d" % (name, len(params), len(bound)))
            continue
        wrong += ["%s: parameter %d is %s, bound as %s" % (name, i, c, p)
                  for i, (c, p) in enumerate(zip(params, bound)) if c != p]
    assert not wrong, "\n".join(wrong)


def test_every_constant_has_the_headers_value():
    header = header_constants()
    assert len(header) >= 40, "the parser found only %d constants" % len(header)
    mirrored = {n: getattr(abi, n) for n in dir(abi) if n.startswith("MN_")}
    assert all(isinstance(v, int) for v in mirrored.values())
    assert set(abi.__all__) >= set(mirrored)
    wrong = ["%s = %d, the header says %d" % (n, v, header[n]) for n, v in sorted(mirrored.items())
             if n in header and v != header[n]]
    assert not wrong, "\n".join(wrong)
    assert {n: v for n, v in mirrored.items() if n not in header} == PYTHON_ONLY


def test_the_structures_have_the_headers_members():
    for c_name, struct in (("mn_options", abi.MnOptions), ("mn_stats", abi.MnStats)):
        members = header_struct(c_name)
        assert len(members) >= 17
        assert [(n, ctypes_kind(t)) for n, t in struct._fields_] == members, c_name


def test_the_module_needs_neither_the_library_nor_torch():
    import subprocess
    import sys
    code = "import sys, mergenet_amd.abi as a; assert 'torch' not in sys.modules and 'numpy' not in sys.modules; " \
           "assert len(a.SIGNATURES) >= 51"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
