"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/adm_hip.h declares (no compute calls -- there is no GPU in the build container)."""
import os
import re

from autodiffusion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "adm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(adm_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    assert _declared_symbols() == sorted(_lib.SIGNATURES)


import pytest


@pytest.mark.parametrize("kind", ["bf16", "f16"])   # libadm_hip.so and its IEEE-half build libadm_hip_f16.so
def test_library_loads_and_exports_every_symbol(kind):
    lib = _lib.load(kind)
    for name in _declared_symbols():
        assert hasattr(lib, name), name
    assert lib.adm_abi_version() == _lib.ABI_VERSION
    assert lib.adm_packed_weight_elems(192, 192, 9) == 6 * 9 * 12 * 512
    assert lib.adm_packed_weight_elems(192, 100, 9) == -1


def test_argument_errors_surface_as_exceptions_without_a_gpu():
    import ctypes as C
    import pytest
    lib = _lib.load()
    st = lib.adm_conv(None, None)
    assert st == -1 and b"null" in lib.adm_last_error()
    with pytest.raises(_lib.AdmError):
        _lib.check(st, "adm_conv")
    assert lib.adm_pack_u8_nhwc(None, None, 1, 3, 8, 8, None) == -1
    co = _lib.StepCoefs()
    assert lib.adm_ddim_step(None, None, None, None, None, None, None, 1, 3, 8, 8, C.byref(co), None) == -1
    # the CU-partition table is host state: registering / forgetting a stream's CU budget needs no GPU
    fake = C.c_void_p(0x1000)
    assert lib.adm_stream_set_cus(fake, 96) == 0 and lib.adm_stream_set_cus(fake, 64) == 0 and lib.adm_stream_set_cus(fake, 0) == 0
    assert lib.adm_stream_set_cus(fake, -1) == -1 and b"ncu" in lib.adm_last_error()
    out = C.c_void_p()
    assert lib.adm_stream_create_cumask(None, 8, C.byref(out)) == -1
    empty = (C.c_uint32 * 8)()
    assert lib.adm_stream_create_cumask(empty, 8, C.byref(out)) == -1 and b"empty mask" in lib.adm_last_error()


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_conv_rejects_out_scale_without_the_fp32_output(kind):
    """out_scale is applied by the fp32 NCHW epilogue only: the library refuses it with a 16-bit output instead of ignoring it
    (argument checks run before any pointer is read, so host placeholders stand in for the device buffers).  The shape is invalid
    on purpose (n = 0, c0 = 31): should the out_scale check ever move or go, a later shape check still refuses the call before
    anything launches."""
    import ctypes as C
    lib = _lib.load(kind)
    a = _lib.ConvArgs()
    a.in0 = a.w_packed = a.bias = a.out = 0x1000
    a.n, a.h, a.w, a.c0, a.cout, a.taps = 0, 16, 16, 31, 32, 9
    a.out_mode, a.out_scale = 0, 2.0 ** -10
    assert lib.adm_conv(C.byref(a), None) == -1   # ADM_E_ARG
    assert b"out_scale" in lib.adm_last_error() and b"out_mode" in lib.adm_last_error()


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_grad_add_rejects_an_odd_size_at_half_resolution(kind):
    """With b_half the kernel reads b[y / 2, x / 2] of an [h / 2, w / 2] operand: an odd h or w indexes past its end, so the
    library refuses it before the launch.  The placeholder pointers are unaligned on purpose: should the odd-size check ever go,
    the alignment check that follows still refuses the call before anything launches."""
    lib = _lib.load(kind)
    for h, w in ((5, 8), (8, 7)):
        assert lib.adm_grad_add(0x1008, 0x1008, 0x1008, 1, h, w, 8, 1, None) != 0
        assert b"adm_grad_add: odd size" in lib.adm_last_error()
    assert lib.adm_grad_add(0x1008, 0x1008, 0x1008, 1, 8, 8, 8, 1, None) != 0 and b"unaligned" in lib.adm_last_error()


def test_header_is_plain_c_and_links_from_a_c_client(tmp_path):
    """include/adm_hip.h compiles as C99 (-pedantic: no C++isms, no torch types) and a C program links against the library."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "client.c"
    src.write_text('#include "adm_hip.h"\n'
                   "int main(void) {\n"
                   "  adm_conv_args a; adm_conv2d_args b; adm_step_coefs c; (void)a; (void)b; (void)c;\n"
                   "  if (adm_conv(0, 0) != ADM_E_ARG) return 2;            /* argument errors need no GPU */\n"
                   "  if (!adm_last_error() || !adm_last_error()[0]) return 3;\n"
                   "  return adm_abi_version() == ADM_ABI_VERSION ? 0 : 1;\n"
                   "}\n")
    libdir = os.path.join(ROOT, "autodiffusion_amd")
    exe = str(tmp_path / "client")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                        "-L", libdir, "-l:libadm_hip.so", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([exe]).returncode == 0
