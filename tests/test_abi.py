"""CPU-side checks of the drop-in boundary: the shared library builds for
gfx950, loads, exports every symbol include/uwspr_hip.h declares, mirrors the
candidate_t layout, and FAILS LOUDLY without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest


def test_library_exports_every_declared_symbol(G):
    N = G.native
    N.build()
    L = N.lib()
    hdr = open(os.path.join(os.path.dirname(N.CSRC), "..", "include", "uwspr_hip.h")).read()
    declared = set(re.findall(r"\b(uwspr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(N.ABI_SYMBOLS), declared ^ set(N.ABI_SYMBOLS)
    for s in declared:
        assert hasattr(L, s), s


def _c_class(decl):
    """the class of one C parameter (or return type) declaration: ptr, str (const char *), i32, i64, size, f64, f32, u32,
    void"""
    d = " ".join(decl.replace("UWSPR_API", " ").replace("extern", " ").replace('"C"', " ").split())
    if "*" in d or "[" in d:
        return "str" if re.match(r"const char \*", d) else "ptr"
    for words, cls in (("long long", "i64"), ("int64_t", "i64"), ("uint64_t", "i64"), ("size_t", "size"), ("double", "f64"),
                       ("float", "f32"), ("uint32_t", "u32"), ("int32_t", "i32"), ("int", "i32"), ("void", "void")):
        if re.search(r"\b%s\b" % words, d):
            return cls
    raise AssertionError("unclassified C declaration %r" % decl)


def _py_class(t):
    """the class of one ctypes type of native.SIGNATURES"""
    if t is None:
        return "void"
    if t is C.c_char_p:
        return "str"
    if t is C.c_void_p or hasattr(t, "contents"):         # (POINTER(x) types have .contents)
        return "ptr"
    assert C.sizeof(C.c_int) == 4 and C.sizeof(C.c_longlong) == 8
    return {C.c_int: "i32", C.c_int32: "i32", C.c_longlong: "i64", C.c_int64: "i64", C.c_size_t: "size", C.c_double: "f64",
            C.c_float: "f32", C.c_uint32: "u32"}[t]


def _declared(text, names, body):
    """{name: (return class, [parameter classes])} of the uwspr_* functions `names` (None: all) declared (body ';') or
    defined (body '{') in C text"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ \*\"]*?)\b(uwspr_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*" + re.escape(body), text):
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        if (names is not None and name not in names) or re.search(r"\b(return|typedef|struct)\b", ret):
            continue
        assert name not in out, name
        out[name] = (_c_class(ret), [] if params in ("", "void") else [_c_class(p) for p in params.split(",")])
    return out


def test_signature_table_matches_the_declarations(G):
    """native.SIGNATURES against the C text, class by class, in order: every function of the header, and every
    diagnostics entry against its extern "C" definition under csrc/.  (A wrong class is a silent truncation: a long long
    passed as a 32-bit int.)  A char * the binding passes as a byte string and a void * are both pointers."""
    N = G.native
    table = {k: (_py_class(r), [_py_class(a) for a in args]) for k, (r, args) in N.SIGNATURES.items()}
    hdr = _declared(open(os.path.join(os.path.dirname(N.CSRC), "..", "include", "uwspr_hip.h")).read(), None, ";")
    assert set(hdr) == set(N.ABI_SYMBOLS), set(hdr) ^ set(N.ABI_SYMBOLS)
    debug = {k for k in N.SIGNATURES if k.startswith("uwspr_debug_")}
    defs = {}
    for f in sorted(os.listdir(N.CSRC)):
        if f.endswith((".hip", ".cpp")):
            for k, v in _declared(open(os.path.join(N.CSRC, f)).read(), debug, "{").items():
                assert k not in defs, k
                defs[k] = v
    assert set(defs) == debug, set(defs) ^ debug
    same = lambda a, b: a == b or {a, b} == {"str", "ptr"}   # noqa: E731
    for name, (ret, params) in dict(hdr, **defs).items():
        pret, pparams = table[name]
        assert pret == ret, (name, "returns", ret, "bound as", pret)
        assert len(params) == len(pparams), (name, params, pparams)
        for k, (c, p) in enumerate(zip(params, pparams)):
            assert same(c, p), (name, "parameter", k, c, "bound as", p)


def test_record_layouts(G):
    N = G.native
    assert N.CAND_DTYPE.itemsize == 48            # candidate_t, lib/candidate_t.h:27-50
    assert N.CAND_DTYPE.fields["shift"][1] == 16 and N.CAND_DTYPE.fields["V1"][1] == 24
    assert N.CAND_DTYPE.fields["p2"][1] == 44
    assert N.HYP_DTYPE.itemsize == 48 and N.DEMOD_DTYPE.itemsize == 2980


def test_parameter_errors_come_before_any_device_use(G):
    """FDR_impl.cc:85-90 exit(-1)s on halfbandwidth > fs/2; the GRC default 187 makes
    the reference read out of bounds.  Both are status codes here, GPU or not."""
    N = G.native
    with pytest.raises(N.UwsprError) as e:
        G.Context(halfbandwidth=200)
    assert e.value.status == -1 and "Half pass bandwidth" in str(e.value)
    with pytest.raises(N.UwsprError) as e:
        G.Context(halfbandwidth=187)
    assert e.value.status == -2
    with pytest.raises(N.UwsprError) as e:
        G.Context(spb=128)
    assert e.value.status == -3


def test_no_gpu_means_loud_failure_not_a_fallback(G):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    N = G.native
    with pytest.raises(N.UwsprError) as e:
        G.Context()
    assert e.value.status == -7 and "no CPU fallback" in str(e.value)


def test_product_never_imports_the_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bad = []
    for base in ("gr-uwspr_amd", "include"):
        for dp, _, files in os.walk(os.path.join(root, base)):
            for f in files:
                if f.endswith((".py", ".hip", ".h", ".cpp", ".cc")):
                    txt = open(os.path.join(dp, f), errors="replace").read()
                    if re.search(r"oracle_py|uwspr_oracle|liboracle|libuwspr_ref", txt):
                        bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_build_is_shared_by_ranks_and_independent_of_the_tree_path(G, tmp_path):
    """What the driver's multi-GPU launch does: N ranks import the package at the same moment, from whatever path the
    tree was copied to.  The library that travelled with the tree must be taken as it is -- no rank recompiles it
    (the stamp holds flags + source contents, not paths or file times), and concurrent callers neither race for the
    output file nor block each other for longer than the check."""
    import subprocess
    import sys
    N = G.native
    N.build()
    before = (os.path.getmtime(N.LIBPATH), os.path.getsize(N.LIBPATH))
    repo = os.path.abspath(os.path.join(os.path.dirname(N.CSRC), ".."))
    other = tmp_path / "another_root"
    os.symlink(repo, other)                               # the same tree under another absolute path
    code = ("import sys, time; sys.path.insert(0, %r); t = time.time(); import gr_uwspr_amd as G; G.build(); "
            "L = G.native.lib(); assert hasattr(L, 'uwspr_ctx_create'); print('%%.1f' %% (time.time() - t))" % str(other))
    procs = [subprocess.Popen([sys.executable, "-c", code], cwd=str(other), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for _ in range(4)]
    for p in procs:
        out, err = p.communicate(timeout=120)
        assert p.returncode == 0, err[-2000:]
        assert float(out.strip().splitlines()[-1]) < 60.0, out       # (an import, not a compile)
    assert (os.path.getmtime(N.LIBPATH), os.path.getsize(N.LIBPATH)) == before
