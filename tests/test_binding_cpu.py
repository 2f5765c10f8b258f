"""CPU-only checks of the ctypes binding: _lib.py reads every argument and return type from the prototypes of
include/dfe_hip.h (no hand-kept table), refuses what it cannot type, and loss_stack.GeomArgs mirrors dfe_geom_args."""
import ctypes
import re

import pytest

from unsupervised_depth_opticalflow_egomotion_amd import _lib, loss_stack

P, I, L, F, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double


def _header_text():
    with open(_lib.HEADER_PATH) as fh:
        return re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)


def _count_parameters(text, name):
    """Top-level commas between the parentheses that follow ``name`` (+ 1); ``(void)`` counts as 0.  Written without the
    parser under test."""
    at = re.search(r"\b%s\s*\(" % name, text).end()
    depth, commas, end = 1, 0, at
    while depth:
        c = text[end]
        depth += (c == "(") - (c == ")")
        commas += c == "," and depth == 1
        end += 1
    return 0 if text[at:end - 1].strip() == "void" else commas + 1


def test_every_declared_symbol_is_typed_from_its_prototype():
    names = _lib.header_symbols()
    sigs = _lib.header_signatures()
    lib, text = _lib.get_lib(), _header_text()
    # no prototype is dropped on the way: every "dfe_name(" of the comment-free header is one
    assert sorted(sigs) == names == sorted(set(re.findall(r"\b(dfe_[a-z0-9_]+)\s*\(", text))) and len(names) >= 93
    for n in names:
        fn = getattr(lib, n)
        assert fn.argtypes is not None, n
        assert len(fn.argtypes) == _count_parameters(text, n), n
        assert (fn.restype, list(fn.argtypes)) == (sigs[n][0], sigs[n][1]), n


PINNED = {
    "dfe_abi_version": (I, []),
    "dfe_error_string": (ctypes.c_char_p, [I]),
    "dfe_scatter_ws_bytes": (L, [L]),
    "dfe_adam_step": (I, [P, P, I, D, D, D, D, D, D, P]),
    "dfe_bias_act_bwd": (I, [P, P, L, P, P, P, I, I, I, I, F, P]),
    "dfe_exact_math_selftest": (I, [P, ctypes.c_ulonglong, P]),
    "dfe_geom_loss_fwd_timed": (I, [P, P, P]),
    "dfe_prepare_triplets_u8": (I, [P, P, P, P, P, P, I, I, I, I, I, P]),
    "dfe_bias_grad_final_multi": (I, [P, P, P, I, I, I, I, P]),
    "dfe_geom_workspace_floats": (L, [P]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signatures(name):
    """One hand-written signature per feature of the header's type language."""
    restype, argtypes = PINNED[name]
    assert _lib.header_signatures()[name] == (restype, argtypes)
    fn = getattr(_lib.get_lib(), name)
    assert fn.restype is restype and list(fn.argtypes) == argtypes


@pytest.mark.parametrize("symbol,proto", [("dfe_x", "int dfe_x(short a, void* stream);"),
                                          ("dfe_y", "int dfe_y(dfe_geom_args a);"),
                                          ("dfe_z", "float dfe_z(int a);")])
def test_untyped_prototypes_are_refused(tmp_path, symbol, proto):
    """A type outside the list, a struct by value, a return type outside the list: DfeError naming the symbol, never an
    untyped function."""
    h = tmp_path / "bad.h"
    h.write_text("#define DFE_ABI_VERSION 3\nint dfe_ok(int n, void* stream);\n" + proto + "\n")
    with pytest.raises(_lib.DfeError, match=symbol):
        _lib.header_signatures(str(h))
    (tmp_path / "junk.h").write_text("int dfe_ok(int n);\nint not_a_prototype;\n")
    with pytest.raises(_lib.DfeError, match="not_a_prototype"):
        _lib.header_signatures(str(tmp_path / "junk.h"))


def test_a_prototype_may_span_lines_and_comments(tmp_path):
    one = tmp_path / "one.h"
    one.write_text("long dfe_f(const float* x, long x_batch_stride, unsigned long long n, float s, void** h, void* stream);\n"
                   "const char* dfe_g(void);\n")
    many = tmp_path / "many.h"
    many.write_text("#ifdef __cplusplus\nextern \"C\" {\n#endif\n#define DFE_N 3 /* a\n two-line comment */\n"
                    "typedef struct { int a, b; } dfe_s;\n"
                    "long dfe_f(const float *x, long x_batch_stride,   /* floats, >= the sample */\n"
                    "           unsigned  long long n, // pairs\n"
                    "           float s, void * * h, void *stream);\n"
                    "const char *\ndfe_g( void );\n#ifdef __cplusplus\n}\n#endif\n")
    sigs = _lib.header_signatures(str(many))
    assert sigs == _lib.header_signatures(str(one)) == {"dfe_f": (L, [P, L, ctypes.c_ulonglong, F, P, P]),
                                                        "dfe_g": (ctypes.c_char_p, [])}
    assert _lib.header_symbols(str(many)) == ["dfe_f", "dfe_g"]


def test_geom_args_mirrors_the_header_struct():
    """loss_stack.GeomArgs against the body of ``dfe_geom_args``: every field's name, order, base type and array extents."""
    text = _header_text()
    max_scales = int(re.search(r"#define\s+DFE_MAX_SCALES\s+(\d+)", text).group(1))
    assert loss_stack.MAX_SCALES == max_scales
    body = re.search(r"typedef\s+struct\s+dfe_geom_args\s*\{(.*?)\}\s*dfe_geom_args\s*;", text, flags=re.S).group(1)
    want = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        m = re.fullmatch(r"((?:const )?(int|float|long))( ?\*)? ?(.+)", decl)
        assert m, decl
        base = "pointer" if m.group(3) else m.group(2)
        for declarator in m.group(4).split(","):
            name, extents = re.fullmatch(r"\s*(\w+)((?:\[\w+\])*)\s*", declarator).groups()
            want.append((name, base, [max_scales if e == "DFE_MAX_SCALES" else int(e) for e in re.findall(r"\[(\w+)\]", extents)]))
    bases = {ctypes.c_int: "int", ctypes.c_float: "float", ctypes.c_long: "long", ctypes.c_void_p: "pointer"}
    have = []
    for name, ctype in loss_stack.GeomArgs._fields_:
        extents = []
        while issubclass(ctype, ctypes.Array):
            extents.append(ctype._length_)
            ctype = ctype._type_
        have.append((name, bases[ctype], extents))
    assert have == want
    assert len(want) == 22 and ("disp", "pointer", [3, max_scales]) in want and ("workspace_floats", "long", []) in want
