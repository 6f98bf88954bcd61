"""The C ABI as include/muygpys_hip.h states it: ctypes signatures and enum constants, read from the header at import.

The header is the only statement of the ABI; nothing here restates it.  Imports ctypes, os and re only (no torch,
nothing of the package): the build's ``python -c`` children load it.  Whatever the reader does not understand is
refused with a ValueError that names the function -- never bound with a guessed type.
"""

import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "muygpys_hip.h")

_BY_VALUE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
_RETURNS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}
_PARAM = re.compile(r"((?:const |unsigned )*\w+)( ?\*+ ?| )\w+")
_DECL = re.compile(r"([\w ]+?)( ?\* ?| )(\w+) ?\(([^()]*)\)")
_header = None


def _param(func: str, decl: str):
    m = _PARAM.fullmatch(decl)
    if not m:
        raise ValueError(f"{func}: cannot read parameter {decl!r}")
    base, stars = m.group(1), m.group(2).strip()
    if stars:
        return ctypes.c_char_p if (base, stars) == ("char", "*") else ctypes.c_void_p
    if base not in _BY_VALUE:
        raise ValueError(f"{func}: parameter {decl!r} is passed by value and is not int / int64_t / double")
    return _BY_VALUE[base]


def parse(text: str):
    """({name: (restype, [argtypes])}, {enum constant: value}) of a header's text."""
    # without /* */ and // comments, preprocessor lines and the opening of extern "C"; white space runs -> one blank
    text = " ".join(chunk.partition("*/")[2] for chunk in ("*/" + text).split("/*"))
    text = " ".join(ln.split("//")[0] for ln in text.split("\n") if not ln.lstrip().startswith("#"))
    text = " ".join(text.split()).replace('extern "C" {', "")
    sigs, consts, seen = {}, {}, {}  # (seen: parameter text -> type; "int k" and "void* stream" recur in every function)
    for stmt in map(str.strip, text.split(";")):
        enum = re.fullmatch(r"enum \w* ?\{(.*)\}", stmt)
        if enum:
            for item in filter(None, (i.strip() for i in enum.group(1).split(","))):
                m = re.fullmatch(r"(\w+) ?= ?(-?\d+)", item)
                if not m:
                    raise ValueError(f"cannot read enum constant {item!r}")
                consts[m.group(1)] = int(m.group(2))
        elif stmt not in ("", "}"):  # (the brace closes extern "C")
            m = _DECL.fullmatch(stmt)
            if not m:
                name = (re.findall(r"(\w+) ?\(", stmt) or [stmt])[0]
                raise ValueError(f"{name}: cannot read declaration {stmt!r}")
            ret, name, params = m.group(1) + m.group(2).strip(), m.group(3), m.group(4).strip()
            if ret not in _RETURNS:
                raise ValueError(f"{name}: return type {ret!r} is not int / int64_t / const char*")
            params = [] if params == "void" else [p.strip() for p in params.split(",")]
            sigs[name] = (_RETURNS[ret], [seen.get(p) or seen.setdefault(p, _param(name, p)) for p in params])
    return sigs, consts


def _parsed():
    global _header
    if _header is None:
        with open(HEADER) as f:
            _header = parse(f.read())
    return _header


def signatures():
    """{name: (restype, [argtypes])} of every function the header declares (parsed once per process)."""
    return _parsed()[0]


def enums():
    """{"MGP_KERNEL_RBF": 0, ...}: every constant of every enum of the header."""
    return _parsed()[1]


def bind(cdll):
    """Set restype and argtypes of every declared function on a loaded library; raises on a symbol it lacks."""
    for name, (restype, argtypes) in signatures().items():
        if not hasattr(cdll, name):
            raise AttributeError(f"{cdll._name} does not export {name}, which include/muygpys_hip.h declares")
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = restype, argtypes
    return cdll
