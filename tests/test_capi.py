"""The C-ABI library builds, loads and exports every entry point declared in include/bm2f.h (no GPU needed)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def _declared():
    src = open(os.path.join(ROOT, "include", "bm2f.h")).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+char\*|int)\s+(m2f_\w+)\s*\(", src, flags=re.M)))


def test_library_exports_header_symbols():
    from bm2f_amd import _native
    lib = _native.load()
    names = _declared()
    assert len(names) >= 6
    for n in names:
        assert hasattr(lib, n), n
    assert set(names) == set(_native.exported_symbols())
    assert lib.m2f_abi_version() == _native.ABI_VERSION
    assert lib.m2f_last_error() == b""


def _header():
    """include/bm2f.h without its comments."""
    src = open(os.path.join(ROOT, "include", "bm2f.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def _kind(param, where):
    """The ctypes kind of one C parameter declaration; an unknown type fails the test."""
    words = param.replace("*", " * ").split()
    if "*" in words:
        if words.count("*") == 1 and words[:words.index("*")] == ["const", "char"]:
            return ctypes.c_char_p
        return ctypes.c_void_p
    types = [w for w in words[:-1] if w != "const"]          # the last word is the parameter's name
    assert len(types) == 1 and types[0] in _SCALARS, f"{where}: unknown parameter type in {param!r}"
    return _SCALARS[types[0]]


def _prototypes():
    """{name: [kind, ...]} of every ``int m2f_*(...)`` prototype of the header."""
    out = {}
    for name, params in re.findall(r"\bint\s+(m2f_\w+)\s*\(([^)]*)\)\s*;", _header()):
        assert name not in out, f"{name} is declared twice"
        params = params.strip()
        out[name] = [] if params in ("", "void") else [_kind(p, name) for p in params.split(",")]
    return out


def test_signature_table_matches_header():
    """_native._SIGNATURES is the only thing between a Python int and the width of a C parameter: every entry must
    equal its prototype in include/bm2f.h, kind for kind, and the two must hold the same names."""
    from bm2f_amd import _native
    protos = _prototypes()
    assert protos.pop("m2f_abi_version") == []               # declared by hand in load(), like m2f_last_error
    assert "m2f_last_error" not in protos and re.search(r"const\s+char\s*\*\s*m2f_last_error\s*\(\s*void\s*\)", _header())
    assert len(protos) >= 90
    assert set(protos) == set(_native._SIGNATURES)
    for name, kinds in protos.items():
        assert kinds == _native._SIGNATURES[name], name


def test_dtype_codes_match_header():
    import torch
    from bm2f_amd import _native
    enum = dict(re.findall(r"\b(M2F_(?:F32|F16|BF16))\s*=\s*(\d+)", _header()))
    assert set(enum) == {"M2F_F32", "M2F_F16", "M2F_BF16"}
    assert _native.DTYPE_CODES == {torch.float32: int(enum["M2F_F32"]), torch.float16: int(enum["M2F_F16"]),
                                   torch.bfloat16: int(enum["M2F_BF16"])}


def test_invalid_args_report_errors_without_gpu():
    from bm2f_amd import _native
    lib = _native.load()
    # null pointers are rejected before any HIP call
    rc = lib.m2f_msda_fwd_f32(None, None, None, None, None, 1, 1, 1, 32, 1, 1, 4, 64, None, None, None)
    assert rc == 1
    assert b"null" in lib.m2f_last_error()


def test_shape_preconditions_rejected_without_gpu():
    """Shape preconditions the kernels rely on are checked in the C entry points themselves (not only by the Python
    callers), before any HIP call: fake aligned pointers never reach a kernel."""
    from bm2f_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(1 << 20)
    # the NHWC FPN merge stores float4s of 2w output columns: odd w is refused
    rc = lib.m2f_upsample2x_add_fwd_nhwc_f32(p, ctypes.c_int64(3 * 7 * 64), p, p, 1, 64, 3, 7, None)
    assert rc == 3 and b"even w" in lib.m2f_last_error()
    # the 16-bit NHWC input-gradient epilogue writes 8 channels per store: output channels % 16 != 0 is refused
    rc = lib.m2f_conv_x3_io(p, 0, 0, p, None, p, 1, 1, 1, 24, 32, 16, 16, 1, 1, p, ctypes.c_int64(1 << 30), None)
    assert rc == 3 and b"output channels" in lib.m2f_last_error()


_P = ctypes.c_void_p(1 << 20)    # aligned, non-null, never dereferenced: every call below returns before the device
_WS = ctypes.c_int64(1 << 20)
# entry point -> arguments with dtype code 99, sized so that no zero-size shortcut returns before the dtype test
_BAD_DTYPE_CALLS = {
    "m2f_bias_act_nchw": (_P, None, _P, 1, 8, 64, 99, 0, None),
    "m2f_relu_bwd_sum": (_P, 1, _P, _P, 64, 99, None),
    "m2f_sum_to_f32": (_P, 1, 64, 99, _P, None),
    "m2f_maxpool3s2_nhwc": (0, _P, _P, _P, 1, 8, 8, 8, 99, None),
    "m2f_maxpool3s2_fwd": (_P, _P, _P, 4, 8, 8, 99, None),
    "m2f_maxpool3s2_bwd": (_P, _P, _P, 4, 8, 8, 99, None),
    "m2f_colsum": (99, _P, 8, 8, _P, _WS, _P, None),
    "m2f_attn_mask_bits": (_P, 99, 1, 4, 1, 8, 8, 8, 8, 0, _P, 2, None),
    "m2f_masked_attn_fwd": (99, _P, _P, _P, _P, 1, 4, 64, 1, 32, 32, 64, 2, 0.25, _P, _P, _P, _WS, None),
    "m2f_masked_attn_bwd": (99, _P, _P, _P, _P, _P, _P, _P, 1, 4, 64, 1, 32, 32, 64, 2, 0.25, _P, _P, _P, _P, _WS, None),
    "m2f_mask_heads_fwd": (99, _P, _P, 1, 4, 32, 1, 8, 8, 0, 0, _P, None, 0, None),
    "m2f_mask_heads_bwd_embed": (99, _P, _P, 1, 4, 256, 16, _P, _P, _WS, None),
    "m2f_mask_heads_bwd_feats": (99, _P, 1, _P, 1, 4, 16, 256, 8, 0, _P, None),
}


@pytest.mark.parametrize("name", sorted(_BAD_DTYPE_CALLS))
def test_unknown_dtype_rejected_without_gpu(name):
    """An element-type code outside M2F_F32 / M2F_F16 / M2F_BF16 is refused as unsupported, with the code in the
    message, by every entry point that tests its dtype before it touches the device."""
    from bm2f_amd import _native
    lib = _native.load()
    rc = getattr(lib, name)(*_BAD_DTYPE_CALLS[name])
    assert rc == 3, lib.m2f_last_error()                     # M2F_EUNSUPPORTED
    assert b"dtype 99" in lib.m2f_last_error()
    assert name.encode() in lib.m2f_last_error()


def test_head_major_wb_rows():
    """msda.head_major_wb: the fused projection's rows regrouped per head -- head m's sampling offsets (L, P, 2)
    then its attention logits (L*P) -- from the two Linear layers (ms_deform_attn.py:59-60), gradients included."""
    import torch
    from bm2f_amd.msda import head_major_wb
    M, L, P, C = 8, 3, 4, 16
    g = torch.Generator().manual_seed(0)
    wo = torch.randn(M * L * P * 2, C, generator=g, requires_grad=True)
    bo = torch.randn(M * L * P * 2, generator=g, requires_grad=True)
    wa = torch.randn(M * L * P, C, generator=g, requires_grad=True)
    ba = torch.randn(M * L * P, generator=g, requires_grad=True)
    w, b = head_major_wb(wo, bo, wa, ba, M)
    LP = L * P
    for m in range(M):
        assert torch.equal(w[m * 3 * LP:m * 3 * LP + 2 * LP], wo[m * 2 * LP:(m + 1) * 2 * LP])
        assert torch.equal(w[m * 3 * LP + 2 * LP:(m + 1) * 3 * LP], wa[m * LP:(m + 1) * LP])
        assert torch.equal(b[m * 3 * LP:m * 3 * LP + 2 * LP], bo[m * 2 * LP:(m + 1) * 2 * LP])
        assert torch.equal(b[m * 3 * LP + 2 * LP:(m + 1) * 3 * LP], ba[m * LP:(m + 1) * LP])
    gw = torch.randn(w.shape, generator=g)
    (w * gw).sum().backward()
    for m in range(M):
        assert torch.equal(wo.grad[m * 2 * LP:(m + 1) * 2 * LP], gw[m * 3 * LP:m * 3 * LP + 2 * LP])
        assert torch.equal(wa.grad[m * LP:(m + 1) * LP], gw[m * 3 * LP + 2 * LP:(m + 1) * 3 * LP])
