"""CPU-side checks of the C-ABI boundary: liblrl.so loads and exports every function that
include/lrl.h declares, each with the header's ctypes signature; the ctypes struct mirror has the C layout.  No compute
calls on a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from lrl import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lrl.h")


def _declared():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(lrl_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("liblrl.so not built")
    lib = C.CDLL(_abi.LIB_PATH)
    missing = [s for s in _declared() if not hasattr(lib, s)]
    assert not missing, missing
    assert lib.lrl_abi_version() == 6


def test_library_matches_the_sources_beside_it():
    """Stale-binary guard: the hash baked into liblrl.so (csrc/Makefile SRC_HASH) equals the hash of the tree's
    sources, and the loader refuses a library whose hash differs."""
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("liblrl.so not built")
    lib = C.CDLL(_abi.LIB_PATH)
    lib.lrl_build_hash.restype = C.c_char_p
    assert lib.lrl_build_hash().decode() == _abi.source_hash()
    assert _abi.lib() is not None
    saved, _abi._lib = _abi._lib, None
    real = _abi.source_hash
    try:
        _abi.source_hash = lambda: "0" * 16
        with pytest.raises(RuntimeError, match="other sources"):
            _abi.lib()
    finally:
        _abi.source_hash, _abi._lib = real, saved


def _prototypes():
    """(return type, name, parameter count) of every prototype, read here without lrl._abi's parser."""
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    out = []
    for ret, name, params in re.findall(r"([\w ]+?[\w\*])\s*\b(lrl_\w+)\s*\(([^()]*)\)\s*;", src):
        out.append((" ".join(ret.split()), name, 0 if params.strip() == "void" else params.count(",") + 1))
    return out


def test_every_function_has_the_headers_signature():
    L = _abi.lib()
    protos = _prototypes()
    assert sorted(name for _, name, _ in protos) == _declared() and len(protos) == 69
    restypes = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "const char*": C.c_char_p}
    for ret, name, nparams in protos:
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nparams, name
        assert fn.restype is restypes[ret], name
    vp, i32, i64, u32, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64
    assert L.lrl_sim_step.argtypes == [vp, vp, u32, vp]
    assert L.lrl_rows_mean_zero_dev.argtypes[1] is i64
    assert L.lrl_sim_create.argtypes == [C.POINTER(_abi.LrlModel), C.POINTER(_abi.LrlEnvParams), i32, i64, u64, i32, vp]
    assert L.lrl_ppo_adaptation_step.argtypes[6:8] == [C.c_double, C.c_float]
    assert L.lrl_ppo_workspace_bytes.restype is i64


def test_a_mistyped_argument_stops_before_the_library():
    """Argument conversion comes before the call: nothing below reaches liblrl (or a device)."""
    L = _abi.lib()
    i32, i64, f32 = C.c_int32, C.c_int64, C.c_float
    gemm = [i32(0), i32(0), i32(1), i32(1), i32(1), None, i64(1), None, i64(1), None, i64(1), None, None, i64(0), None,
            None, i64(0), None]
    assert L.lrl_gemm_f32.argtypes[6] is i64
    gemm[6] = i32(1)  # lda
    with pytest.raises(C.ArgumentError):
        L.lrl_gemm_f32(*gemm)
    assert L.lrl_gae.argtypes[6] is f32
    with pytest.raises(C.ArgumentError):  # gamma
        L.lrl_gae(None, None, None, None, i32(1), i32(1), C.c_double(0.99), f32(0.95), None, None, None, None)
    with pytest.raises(C.ArgumentError):  # lrl_metrics_view* out
        L.lrl_sim_metrics_tensors(None, C.c_void_p())


def test_a_64_bit_address_passes_as_a_bare_int():
    import numpy as np
    a = np.random.default_rng(3).standard_normal(1001)
    addr = a.ctypes.data
    print("buffer address above 2^32:", addr >= 1 << 32)  # (the c_void_p slot carries it either way)
    assert _abi.lib().lrl_np_sum_f64.argtypes == [C.c_void_p, C.c_int64]
    assert _abi.lib().lrl_np_sum_f64(addr, len(a)) == np.sum(a)


def test_signature_parser_refuses_what_it_cannot_map():
    ok = "int32_t lrl_fine(const float* a, int64_t n, lrl_tensor* out);"
    assert _abi.signatures(ok) == {"lrl_fine": (C.c_int32, [C.c_void_p, C.c_int64, C.POINTER(_abi.LrlTensor)])}
    for bad in ("int32_t lrl_odd(const float* a, size_t n);", "int32_t lrl_odd(int32_t (*callback)(void));",
                "int32_t lrl_odd(float v[3]);", "size_t lrl_odd(void);"):
        with pytest.raises(RuntimeError, match="lrl_odd"):
            _abi.signatures(ok + "\n" + bad)


def test_struct_layout_matches_header(tmp_path):
    mirrors = sorted(_abi.MIRRORS)
    assert len(mirrors) == 14
    code = r"""
#include <stdio.h>
#include <stddef.h>
#include "lrl.h"
int main(){printf("%zu %zu %zu %zu %zu %zu\n", sizeof(lrl_model), sizeof(lrl_env_params), sizeof(lrl_tensor),
 offsetof(lrl_env_params, noise_vec), offsetof(lrl_env_params, max_episode_length), sizeof(lrl_rollout_store));
printf("%zu %zu %zu %zu %zu %zu\n", sizeof(lrl_ppo_net), offsetof(lrl_ppo_net, total), sizeof(lrl_ppo_batch),
 offsetof(lrl_ppo_batch, batch), sizeof(lrl_ppo_hparams), sizeof(lrl_ppo_ctrl));
printf("%zu %zu\n", offsetof(lrl_ppo_batch, hist_ld), offsetof(lrl_rollout_store, hist_ld));
printf("%zu %zu %zu\n", sizeof(lrl_dev_curriculum), offsetof(lrl_dev_curriculum, nz), offsetof(lrl_dev_curriculum, draws));
printf("%zu %zu %zu %zu %zu %zu\n", sizeof(lrl_gemm_desc), offsetof(lrl_gemm_desc, splits), offsetof(lrl_gemm_desc, A),
 offsetof(lrl_gemm_desc, lda), offsetof(lrl_gemm_desc, workspace_floats), offsetof(lrl_gemm_desc, splits_out));
"""
    code += "".join(f'printf("%zu\\n", sizeof({name}));\n' for name in mirrors) + "return 0;}\n"
    exe = str(tmp_path / "lrl_layout_check")
    src = exe + ".c"
    with open(src, "w") as f:
        f.write(code)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    out = [int(x) for x in subprocess.check_output([exe]).split()]
    assert out == [C.sizeof(_abi.LrlModel), C.sizeof(_abi.LrlEnvParams), C.sizeof(_abi.LrlTensor),
                   _abi.LrlEnvParams.noise_vec.offset, _abi.LrlEnvParams.max_episode_length.offset,
                   C.sizeof(_abi.LrlRolloutStore), C.sizeof(_abi.LrlPpoNet), _abi.LrlPpoNet.total.offset,
                   C.sizeof(_abi.LrlPpoBatch), _abi.LrlPpoBatch.batch.offset, C.sizeof(_abi.LrlPpoHparams),
                   _abi.PPO_CTRL_BYTES, _abi.LrlPpoBatch.hist_ld.offset, _abi.LrlRolloutStore.hist_ld.offset,
                   C.sizeof(_abi.LrlDevCurriculum), _abi.LrlDevCurriculum.nz.offset, _abi.LrlDevCurriculum.draws.offset, C.sizeof(_abi.LrlGemmDesc), _abi.LrlGemmDesc.splits.offset,
                   _abi.LrlGemmDesc.A.offset, _abi.LrlGemmDesc.lda.offset, _abi.LrlGemmDesc.workspace_floats.offset,
                   _abi.LrlGemmDesc.splits_out.offset] + [C.sizeof(_abi.MIRRORS[name]) for name in mirrors]


def test_product_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from lrl.env import LeggedRobotEnv
    with pytest.raises(RuntimeError):
        LeggedRobotEnv("cuda:0")
