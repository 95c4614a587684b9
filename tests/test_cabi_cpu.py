"""CPU checks of the drop-in boundary: the C-ABI library loads here (no GPU), exports every symbol that
include/smsut_hip.h declares and nothing else, every definition is compiled against that header, and the binding _hip.py reads
from it agrees with this file's own reading argument-for-argument and refuses a tensor that does not fit its parameter.
No compute entry point is called."""
import ctypes
import os
import re

import pytest

import __graft_entry__ as ge

HEADER = os.path.join(ge.ROOT, "include", "smsut_hip.h")


@pytest.fixture(scope="module")
def built():
    ge.build()
    assert os.path.exists(ge.LIB)
    return ctypes.CDLL(ge.LIB)


def header_decls():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(int|int64_t)\s+(smsut_\w+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S):
        ret, name, args = m.group(1), m.group(2), m.group(3)
        kinds = []
        for a in [a.strip() for a in args.split(",") if a.strip() and a.strip() != "void"]:
            if "*" in a:
                kinds.append("p")
            elif a.startswith("int64_t"):
                kinds.append("l")
            elif a.startswith("int"):
                kinds.append("i")
            elif a.startswith("float"):
                kinds.append("f")
            elif a.startswith("double"):
                kinds.append("d")
            else:
                raise AssertionError(f"unparsed argument {a!r} in {name}")
        decls[name] = (ret, "".join(kinds))
    return decls


def test_library_exports_every_declared_symbol(built):
    decls = header_decls()
    assert len(decls) >= 50
    for name in decls:
        assert hasattr(built, name), f"{name} declared in include/smsut_hip.h but not exported"


def test_ctypes_table_matches_header(built):
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip
    decls = header_decls()
    assert set(_hip.SIGNATURES) == set(decls), set(_hip.SIGNATURES) ^ set(decls)
    for name, sig in _hip.SIGNATURES.items():
        got = sig.replace(" ", "").replace("s", "p")          # the stream is a void*
        assert got == decls[name][1], (name, got, decls[name][1])
        assert (decls[name][0] == "int64_t") == (name in _hip._RET_I64), name
    _hip.load()


_SLABS = {"smsut_conv2d_wgrad_mfma_slabs", "smsut_conv2d_wgrad_pair_slabs"}     # take a stream, return a count of split slabs


def test_status_follows_from_the_trailing_stream():
    """An entry point returns a status exactly when its last parameter is ``void* stream`` (it enqueues work), but for the two
    measurement entry points; read here from the header text, not through _hip's parser."""
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    seen = 0
    for m in re.finditer(r"\b(?:int|int64_t)\s+(smsut_\w+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S):
        name, streamed = m.group(1), re.search(r"(^|,)\s*void\s*\*\s*stream\s*$", m.group(2)) is not None
        assert (name in _hip._NO_STATUS) == (not streamed or name in _SLABS), name
        seen += 1
    assert seen == len(header_decls()) and _hip._NO_STATUS <= set(header_decls())
    assert _SLABS <= set(header_decls())


def test_library_exports_nothing_undeclared(built):
    """The other direction of test_library_exports_every_declared_symbol: every defined dynamic symbol with the C name smsut_* is
    declared in the header (the internal C++ interfaces are mangled and do not match).  Read with the llvm-readelf that ships
    with the compiler."""
    import subprocess
    llvm_bin = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(ge.HIPCC))), "lib", "llvm", "bin")
    out = subprocess.check_output([os.path.join(llvm_bin, "llvm-readelf"), "--dyn-syms", "--wide", ge.LIB], text=True)
    rows = [ln.split() for ln in out.splitlines()]
    exported = {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}
    smsut = {n for n in exported if n.startswith("smsut_")}
    decls = header_decls()
    assert len(smsut) >= 50 and any(n.startswith("_Z") and "smsut_" in n for n in exported)       # the listing was read
    assert smsut <= set(decls), sorted(smsut - set(decls))


def test_every_definition_is_compiled_against_the_header():
    """Each csrc/*.hip that defines entry points (an ``extern "C"``) includes include/smsut_hip.h, directly or through the project's
    own headers, so a definition whose parameter list drifts from its declaration does not compile ("conflicting types")."""
    def closure(path, seen):
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M):
            for d in (os.path.dirname(path), os.path.join(ge.ROOT, "include")):
                f = os.path.join(d, inc)
                if os.path.exists(f) and f not in seen:
                    seen.add(f)
                    closure(f, seen)
        return seen
    units = [os.path.join(ge.CSRC, f) for f in sorted(os.listdir(ge.CSRC)) if f.endswith(".hip")]
    defining = [u for u in units if 'extern "C"' in open(u).read()]
    assert len(defining) >= 18
    for u in defining:
        assert HEADER in closure(u, set()), f"{os.path.basename(u)} defines entry points without seeing smsut_hip.h"


@pytest.fixture()
def recorded(built, monkeypatch):
    """``recorded(name)`` replaces the bound library function by a recorder and returns the list of argument tuples it was entered
    with: nothing of the library runs."""
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip
    lib = _hip.load()

    def install(name):
        calls = []
        getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a: calls.append(a) or 0)
        return calls
    return install


def test_call_refuses_a_tensor_that_does_not_fit_its_parameter(recorded):
    import torch
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip
    f32, f16, u8 = torch.zeros(8), torch.zeros(8, dtype=torch.float16), torch.zeros(8, dtype=torch.uint8)
    add_act, expand, restail = recorded("smsut_add_act"), recorded("smsut_tta_expand"), recorded("smsut_restail_fwd_hs")
    # int smsut_add_act(const float* a, const float* b /*nullable*/, float* y, int64_t n, float slope, void* stream)
    with pytest.raises(_hip.SmsutHipError, match=r"smsut_add_act: argument 0 \(`const float\* a`\).*float32.*float16"):
        _hip.call("smsut_add_act", f16, None, f32, 8, 0.1, 0)
    with pytest.raises(_hip.SmsutHipError, match=r"smsut_add_act: argument 1 \(`const float\* b`\).*float32.*float16"):
        _hip.call("smsut_add_act", None, f16, None, 8, 0.1, 0)
    with pytest.raises(_hip.SmsutHipError, match=r"smsut_add_act: argument 3 \(`int64_t n`\).*number.*float32 tensor"):
        _hip.call("smsut_add_act", None, None, None, f32, 0.1, 0)
    with pytest.raises(_hip.SmsutHipError, match=r"smsut_add_act: argument 5 \(`void\* stream`\).*stream"):
        _hip.call("smsut_add_act", None, None, None, 8, 0.1, f32)
    # int smsut_tta_expand(const uint8_t* img, float* out, const int* transforms, int T, int N, int H, int W, void* stream)
    with pytest.raises(_hip.SmsutHipError, match=r"smsut_tta_expand: argument 1 \(`float\* out`\).*float32.*uint8"):
        _hip.call("smsut_tta_expand", None, u8, None, 1, 1, 2, 4, 0)
    # a `void*` parameter takes any dtype: the fp16 tensor gets as far as the device check
    with pytest.raises(_hip.SmsutHipError, match="need tensors on a HIP device"):
        _hip.call("smsut_restail_fwd_hs", f16, *[None] * 10, 1, 2, 4, 0.1, 0)
    with pytest.raises(_hip.SmsutHipError, match="need tensors on a HIP device"):
        _hip.call("smsut_add_act", f32, None, f32, 8, 0.1, 0)                 # correctly typed, on the CPU
    assert add_act == [] and expand == [] and restail == []                  # the library was never entered
    # None (nullable) and plain ints (host addresses) pass in pointer slots, as they are
    assert _hip.call("smsut_add_act", 4096, None, 8192, 8, 0.1, 0) == 0
    assert add_act == [(4096, None, 8192, 8, 0.1, 0)]
    with pytest.raises(TypeError):                                           # a wrong argument count stays ctypes' to report
        _hip.call("smsut_in_chunks", 32, 65536)


def test_support_queries_and_workspace_sizes(built):
    """Pure host-side helpers (no device work): eligibility of the MFMA path and workspace sizing."""
    f = built.smsut_conv2d_mfma_supported
    assert f(3, 1, 1, 16, 16) == 1 and f(1, 1, 0, 256, 128) == 1
    assert f(3, 1, 1, 1, 8) == 0 and f(3, 2, 1, 16, 16) == 0 and f(5, 1, 2, 16, 16) == 0 and f(3, 1, 0, 16, 16) == 0
    assert built.smsut_convT2x2_mfma_supported(256, 128) == 1 and built.smsut_convT2x2_mfma_supported(6, 8) == 0
    built.smsut_conv2d_wgrad_mfma_ws.restype = ctypes.c_int64
    ws = built.smsut_conv2d_wgrad_mfma_ws(32, 256, 256, 16, 16, 3)
    assert ws % (9 * 16 * 16) == 0 and 0 < ws // (9 * 16 * 16) <= 1024
    ws_big = built.smsut_conv2d_wgrad_mfma_ws(32, 16, 16, 256, 256, 3)
    assert ws_big * 4 <= 32 << 20            # split slabs stay bounded (WGRAD_CAP_MFLOATS in conv_mfma.hip: 8M floats)
    assert built.smsut_in_chunks(32, 65536, 16) >= 32


def test_product_path_fails_loudly_without_gpu_or_library(monkeypatch):
    import torch
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip, ops
    if torch.cuda.is_available():
        pytest.skip("CPU-only check")
    x = torch.zeros(1, 4, 8, 8)
    w = ops.new_weight(4, 4, 3, 3)
    with pytest.raises(_hip.SmsutHipError):
        ops.conv2d(x, w, None, 1, 1)                       # CPU tensors are refused: no fallback
    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setattr(_hip, "LIB_PATH", "/nonexistent/libsmsut_hip.so")
    with pytest.raises(_hip.SmsutHipError):
        _hip.load()


def test_wino_kernels_leave_m0_to_the_dma_statements(tmp_path):
    """csrc/conv_wino.hip issues its LDS-DMA copies from inline assembly that writes M0 and does not restore it (the compiler
    reserves M0; see the comment at glds16).  That is only sound while nothing else in those kernels touches M0: every mention of
    m0 in the generated ISA must be the `s_mov_b32 m0, sN` of such a statement, followed by its s_nop and global_load_lds."""
    import subprocess
    out = tmp_path / "conv_wino.s"
    subprocess.check_call([ge.HIPCC, *ge.FLAGS, "-I", os.path.join(ge.ROOT, "include"), "--cuda-device-only", "-S",
                           os.path.join(ge.CSRC, "conv_wino.hip"), "-o", str(out)])
    lines = [ln.split(";")[0].strip() for ln in open(out)]
    lines = [ln for ln in lines if ln and not ln.startswith(".")]
    uses = [i for i, ln in enumerate(lines) if re.search(r"\bm0\b", ln)]
    assert len(uses) > 100                                     # the DMA statements exist (15 per chunk loop and instantiation)
    for i in uses:
        assert re.fullmatch(r"s_mov_b32 m0, s\d+", lines[i]), lines[i]
        assert lines[i + 1].startswith("s_nop") and lines[i + 2].startswith("global_load_lds_dwordx4"), lines[i:i + 3]
    n_dma = sum(ln.startswith("global_load_lds_dwordx4") for ln in lines)
    assert n_dma == len(uses)


def test_weight_gradient_workspace_covers_every_kernel_plan():
    """Host logic only (no launch): the workspace the callers allocate from ``smsut_conv2d_wgrad_mfma_ws`` / ``_sc_ws`` must hold the split
    slabs of whichever kernel takes the shape -- the LDS-staged ones or the register-row one (csrc/conv_wgrad_rr.hip plans its own split
    count) -- and ``smsut_conv2d_wgrad_sc_supported`` covers the 16-channel slabs since r04."""
    import ctypes
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip as H
    lib = H.load()
    lib.smsut_conv2d_wgrad_mfma_ws.restype = ctypes.c_int64
    lib.smsut_conv2d_wgrad_sc_ws.restype = ctypes.c_int64
    for n in (1, 3, 16, 32):
        for (h, w) in ((256, 256), (128, 128), (64, 64), (20, 48), (16, 16), (8, 8), (4, 4)):
            for (ci, co) in ((16, 16), (32, 16), (16, 32), (32, 32), (64, 32), (128, 128), (256, 256), (8, 16), (48, 80)):
                need = lib.smsut_conv2d_wgrad_mfma_ws(n, h, w, ci, co, 3)
                assert need >= 9 * ci * co, (n, h, w, ci, co, need)
                assert need % (9 * ci * co) == 0 or need > 9 * ci * co
                assert need <= 64 * (1 << 20), (n, h, w, ci, co, need)          # bounded slabs (sum_splits re-reads them)
                if lib.smsut_conv2d_wgrad_sc_supported(n, h, w, ci, co):
                    assert lib.smsut_conv2d_wgrad_sc_ws(n, h, w, ci, co) >= 10 * ci * co
    assert lib.smsut_amax_blocks(16, 65536, 16) > 0 and lib.smsut_amax_blocks(0, 65536, 16) == 0
    assert lib.smsut_conv2d_wgrad_sc_supported(16, 256, 256, 32, 16) == 1            # r04: the register-row kernel carries the extra tile
    assert lib.smsut_conv2d_wgrad_sc_supported(16, 128, 128, 16, 32) == 1
    assert lib.smsut_conv2d_wgrad_sc_supported(16, 256, 256, 48, 80) == 0


# Environment switches whose experiments ended: the library and the package read none of them any more.
_RETIRED_ENV = """
    CONV_PERSISTENT CONV_K8 CONV_N8 DENSE_PLANES F16_CK32 FUSE_SHORTCUT FUSE_SHORTCUT_F16 FUSE_SHORTCUT_DGRAD
    FUSE_SHORTCUT_DGRAD_F16 FUSE_SHORTCUT_WGRAD FUSE_SHORTCUT_WGRAD_F16 F16_STORE PLANE_WGRAD WGRAD_PAIR WGRAD_RR WINOGRAD_L
    CONVT_PS STEM IN_ONE_CHUNK IN_SLABS WINOGRAD_WG F16_TH16 CFG_F16 WINO_L_MIN_K WGRAD_TARGET11 WGRAD_TARGET
    WGRAD_CAP_MFLOATS RR_TARGET RR_TARGET4 RR_RCMAX IN_SLAB_WGS WINO_WGS_PER_CU CUS P_WGS_PER_CU WINO_NTN RR_V32 LOG_CONV
    ONE_PASS_CONCAT INAFF_CONV2 POOL_SKIP THIN_1X1 REMASK_TAIL FUSED_BWD_STATS HS_INAFF INAFF_MIN_CO FIN_MASK
    FORCE_GENERIC_CONV WINO_PREPARED""".split()
_RETIRED_OPS_FLAGS = """ONE_PASS_CONCAT INAFF_CONV2 POOL_SKIP THIN_1X1 REMASK_TAIL FUSED_BWD_STATS HS_INAFF F16_STORE INAFF_MIN_CO
    FIN_MASK FORCE_GENERIC_CONV WINO_PREPARED""".split()


def test_library_reads_one_environment_variable():
    """Which kernel runs depends on the call's arguments alone, except for SMSUT_WINOGRAD (the direct forms as the reference the
    Winograd forms are tested against): ``getenv`` appears once in csrc/, inside that helper, and no retired switch is named in
    csrc/ or in the package's Python files."""
    pkg = os.path.dirname(ge.CSRC)
    csrc = {f: open(os.path.join(ge.CSRC, f)).read() for f in sorted(os.listdir(ge.CSRC)) if f.endswith((".hip", ".h"))}
    calls = [(f, ln) for f, txt in csrc.items() for ln in txt.splitlines() if "getenv" in ln]
    assert len(calls) == 1 and calls[0][0] == "common.h" and 'getenv("SMSUT_WINOGRAD")' in calls[0][1], calls
    helper = re.search(r"inline bool winograd_on\(\) \{(.*?)\n\}", csrc["common.h"], flags=re.S)
    assert helper and "getenv" in helper.group(1)
    env = re.compile(r"\bSMSUT_(%s)\b" % "|".join(_RETIRED_ENV))
    flags = re.compile(r"\b(%s)\b" % "|".join(_RETIRED_OPS_FLAGS))
    py = {}
    for d, _, files in os.walk(pkg):
        py.update({os.path.join(d, f): open(os.path.join(d, f)).read() for f in files if f.endswith(".py")})
    assert py
    for path, txt in [*((os.path.join(ge.CSRC, f), t) for f, t in csrc.items()), *py.items()]:
        assert not env.search(txt), (path, env.search(txt).group(0))
        if path.endswith(".py"):
            assert not flags.search(txt), (path, flags.search(txt).group(0))
