"""The Julia binding (flight.jl_amd/julia/FlightBatch.jl) cannot be executed here (no Julia toolchain), so it is checked by
inspection: every capitalised identifier the module uses unqualified must be imported, defined in the module, or a name of
Julia's Base / Core — the class of error (`UndefVarError` at `using FlightBatch`) a missing import produces."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "flight.jl_amd", "julia", "FlightBatch.jl")

# names every Julia session has (Base / Core exports the shim uses)
BASE = {"Cint", "Cdouble", "Cstring", "Cvoid", "Ptr", "Ref", "Int", "Int32", "Int64", "UInt8", "UInt32", "Float32", "Float64", "Bool",
        "Integer", "Real", "Symbol", "Vector", "Matrix", "Array", "Dict", "NTuple", "Any", "ENV", "C_NULL", "Base", "Union", "Nothing", "DimensionMismatch"}


def _code_only(src):
    """the source with string literals (single- and triple-quoted, possibly multi-line) emptied and comments removed"""
    out, i, n = [], 0, len(src)
    while i < n:
        if src.startswith('"""', i):
            j = src.find('"""', i + 3)
            out.append('""'); i = j + 3
        elif src[i] == '"':
            j = i + 1
            while src[j] != '"':
                j += 2 if src[j] == "\\" else 1
            out.append('""'); i = j + 1
        elif src[i] == "#":
            j = src.find("\n", i)
            i = n if j < 0 else j
        else:
            out.append(src[i]); i += 1
    return "".join(out)


def _imports(code):
    names, paths = set(), []
    for m in re.finditer(r"^\s*(?:using|import)\s+([\w.]+)\s*:\s*(.+)$", code, flags=re.M):
        mod, items = m.group(1), [s.strip() for s in m.group(2).split(",")]
        names.update(i for i in items if i)
        paths.append((mod, items))
    return names, paths


def test_every_capitalised_identifier_is_in_scope():
    code = _code_only(open(SHIM, encoding="utf-8").read())
    imported, _ = _imports(code)
    defined = set(re.findall(r"^\s*(?:mutable\s+)?struct\s+(\w+)", code, flags=re.M))
    defined |= set(re.findall(r"^\s*module\s+(\w+)", code, flags=re.M))
    for m in re.finditer(r"^\s*const\s+(.+?)\s*=", code, flags=re.M):        # const A, B, C = ...
        defined.update(s.strip() for s in m.group(1).split(","))
    for m in re.finditer(r"\(;\s*([^)]*)\)\s*=", code):                      # (; a, b) = x  destructuring
        defined.update(t.strip() for t in m.group(1).split(","))
    body = re.sub(r"^\s*(?:using|import)\s.*$", "", code, flags=re.M)
    body = re.sub(r"\b\w+::", "", body)                                       # field / argument declarations `name::Type`
    # unqualified uses: an identifier starting with an upper-case ASCII letter that is not a field / submodule access (`x.Name`),
    # not a keyword argument name (`Name = ...` inside a call is lower-case in this file) and not a type parameter
    used = set(m.group(1) for m in re.finditer(r"(?<![\w.!:])([A-Z][A-Za-z0-9_]*)\b", body))
    type_params = set(re.findall(r"where\s*\{?\s*([A-Z]\w*)", body))
    unknown = sorted(n for n in used - imported - defined - BASE - type_params)
    assert not unknown, f"FlightBatch.jl uses names that are neither imported nor defined: {unknown}"
    # the three failures this test was written for
    for name in ("WA", "ECEF", "NED", "Cessna172Sv0", "Cessna172Xv2"):
        assert name in imported, name
    assert not re.search(r"^\s*put!\(", code, flags=re.M), "the shim must not shadow Base.put!"
    assert "pathof(Geodesy" not in code   # pathof() of a submodule is `nothing`
