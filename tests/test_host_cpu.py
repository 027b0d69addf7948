"""CPU-only checks of the host side: C-ABI surface, module schema, error behaviour, schedule logic."""
import os
import subprocess

import numpy as np
import pytest
import torch

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib
from conv_tasnet_amd.solver import _HalvingSchedule
from conftest import load_golden, ROOT
from oracle import ctn_oracle as O


def test_library_exports_every_symbol_the_header_declares():
    protos = _lib.parse_header()
    assert len(protos) >= 27
    out = subprocess.run(["nm", "-D", "--defined-only", ctn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    missing = sorted(set(protos) - exported)
    assert not missing, missing
    ctn.lib.load()      # dlopen + bind every prototype; no compute


def test_host_side_entry_points_without_gpu():
    assert ctn.lib.ctn_version() >= 100
    assert ctn.lib.ctn_padded_frames(3199) == 3200 and ctn.lib.ctn_padded_frames(64) == 64
    assert ctn.lib.ctn_padded_frames(1) == 64
    assert ctn.lib.ctn_pw_stats_parts(8, 512, 3200) >= 100
    assert ctn.lib.ctn_pw_wgrad_workspace(8, 512, 256, 3200) % (512 * 256 * 4) == 0
    assert ctn.lib.ctn_dw_bwd_rows(3, 1) == 8 and ctn.lib.ctn_dw_bwd_rows(3, 0) == 3
    assert ctn.lib.ctn_sisnr_workspace(8, 2, 32000) == 8 * ctn.lib.ctn_sisnr_chunks(32000) * 12 * 8
    assert ctn.lib.ctn_last_error() is not None


def test_bad_arguments_return_error_codes_not_crashes():
    # null pointers / bad sizes are rejected before any launch, so this is safe without a GPU
    rc = ctn.lib.ctn_pw_gemm(0, 0, 0, 1, 4, 4, 4, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert rc == -1 and b"null" in ctn.lib.ctn_last_error()
    rc = ctn.lib.ctn_dw_fwd(16, 16, 16, 1, 4, 8, 8, 99, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert rc == -1 and b"kernel size" in ctn.lib.ctn_last_error()
    with pytest.raises(ctn.CtnError):
        ctn.lib.call("ctn_im2col", 0, 0, 1, 100, 20, 20, 9, 64, 0)


def test_delay_hook_parses_and_refuses_out_of_range_arguments_before_any_launch():
    """The schedule-perturbation hook (tests/sched_harness.py): the header parses with its three prototypes, a delay outside
    [0, 20000] microseconds or a group below -1 is refused with a message, and arming / reading the counter launches nothing (this
    runs without a GPU)."""
    import ctypes
    protos = _lib.parse_header()
    assert protos["ctn_delay"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int], ["stream", "micros"])
    assert protos["ctn_delay_arm"] == (ctypes.c_int, [ctypes.c_int, ctypes.c_int], ["group", "micros"])
    assert protos["ctn_delay_groups"] == (ctypes.c_int, [], [])
    L = ctn.lib.load()
    try:
        assert L.ctn_delay_arm(-1, 0) == 0 and L.ctn_delay_groups() == 0         # (resets the count that an earlier sweep left)
        for micros in (-1, 20001, 2 ** 31 - 1):
            assert L.ctn_delay(0, micros) == -1 and ctn.lib.ctn_last_error().startswith(b"ctn_delay: micros"), micros
            assert L.ctn_delay_arm(0, micros) == -1 and ctn.lib.ctn_last_error().startswith(b"ctn_delay_arm:"), micros
        assert L.ctn_delay_arm(-2, 100) == -1 and b"group" in ctn.lib.ctn_last_error()
        assert L.ctn_delay_groups() == 0                    # a refused arm leaves the hook off
        assert L.ctn_delay_arm(-1, 0) == 0 and L.ctn_delay_groups() == 0 and L.ctn_delay_groups() == 0
        assert L.ctn_delay_arm(3, 20000) == 0 and L.ctn_delay_groups() == 0      # armed, no launch group issued, disarmed again
    finally:
        L.ctn_delay_groups()


def test_schedule_harness_poisons_every_uninitialised_allocation_the_package_makes():
    """tests/sched_harness.py can only show a race through a buffer that was poisoned: every function through which the package gets
    uninitialised memory must be one that poisoned_allocations() wraps, and the wrappers must come off again."""
    import re
    import sched_harness as SH
    pkg = os.path.join(ROOT, "conv-tasnet_amd")
    used = set()
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            used |= {"torch." + m for m in re.findall(r"\btorch\.(empty\w*)\(", src)}
            used |= {"Tensor." + m for m in re.findall(r"\.(new_empty\w*)\(", src)}
    assert "torch.empty" in used and "torch.empty_like" in used
    assert used <= {"torch." + n for n in SH.UNINITIALISED} | {"Tensor." + n for n in SH.UNINITIALISED_METHODS}, used
    before = [getattr(torch, n) for n in SH.UNINITIALISED] + [getattr(torch.Tensor, n) for n in SH.UNINITIALISED_METHODS]
    with SH.poisoned_allocations():
        assert all(getattr(torch, n).__name__ == "alloc" for n in SH.UNINITIALISED)
        assert all(getattr(torch.Tensor, n).__name__ == "alloc" for n in SH.UNINITIALISED_METHODS)
        x = torch.zeros(3)
        assert torch.empty_like(x).shape == x.new_empty(3).shape == torch.empty(3).shape      # CPU tensors pass through untouched
    assert before == [getattr(torch, n) for n in SH.UNINITIALISED] + [getattr(torch.Tensor, n) for n in SH.UNINITIALISED_METHODS]


def test_tune_refuses_the_removed_keys_and_keeps_the_others():
    """The keys of the removed persistent GEMM and chained weight gradients are unknown keys now; the switches that stayed still
    take their default values (read from the sources: the mirror of the cLN dispatch and the lines that parse the environment)."""
    import re
    import norm_oracle as NO
    from conftest import DEFAULT_ARITH
    from conv_tasnet_amd import ops
    csrc = os.path.join(ROOT, "conv-tasnet_amd", "csrc")
    cln, dw = (open(os.path.join(csrc, f)).read() for f in ("ctn_cln.hip", "ctn_dw.hip"))
    assert "int g_ctn_cln_fr = %d;" % NO.DEFAULT_FR in cln and "int g_ctn_cln_lean = %d;" % NO.DEFAULT_LEAN in cln
    defaults = {b"arith": ops._ARITH_NAMES.index(DEFAULT_ARITH), b"cln_fr": NO.DEFAULT_FR, b"cln_lean": NO.DEFAULT_LEAN,
                b"cln_fuse": int(re.search(r"g_ctn_cln_fuse = \(e && [^;]*\? \*e - '0' : (\d);", cln).group(1)),
                b"gln_fuse": int(re.search(r"g_ctn_gln_fuse = \(e && [^;]*\? \*e - '0' : (\d);", dw).group(1))}
    tune = ctn.lib.load().ctn_tune
    try:
        for key in (b"b3_ws", b"b3_ws_blocks", b"wgrad_chain"):
            for value in (0, 1):
                assert tune(key, value) == -1, key
                assert key in ctn.lib.ctn_last_error(), (key, ctn.lib.ctn_last_error())
        for key, value in defaults.items():
            assert tune(key, value) == 0, (key, value, ctn.lib.ctn_last_error())
    finally:
        for key, value in defaults.items():
            tune(key, value)


def _dw_call(name, **kw):
    """A depthwise entry point on fake 16-byte-aligned pointers with complete, valid arguments except for `kw` (by the header's
    parameter names): such a call must be refused before any HIP call.  -> (status, message)"""
    dflt = {"M": 1, "H": 4, "K": 8, "Kp": 8, "P": 3, "dilation": 1, "causal": 0, "fused": 1, "sums2_nparts": 1, "stream": 0}
    names = ctn.lib.protos[name][2]
    assert set(kw) <= set(names), (name, kw)
    rc = getattr(ctn.lib.load(), name)(*[kw[nm] if nm in kw else dflt.get(nm, 16) for nm in names])
    return rc, ctn.lib.ctn_last_error().decode()


@pytest.mark.parametrize("name,kw", [
    ("ctn_dw_fwd_cln", {"P": 99}),
    ("ctn_dw_bwd_gln2", {"P": 99}),
    ("ctn_dw_bwd_gln2", {"ms1": 0}),
    ("ctn_dw_bwd_cln", {"P": 2, "dilation": 3, "causal": 0}),
    ("ctn_dw_bwd_cln", {"mean1": 0}),
    ("ctn_dw_bwd", {"fused": 4}),
    ("ctn_dw_bwd", {"fused": -1}),
])
def test_depthwise_entry_points_name_themselves_when_they_refuse(name, kw):
    rc, msg = _dw_call(name, **kw)
    assert rc == -1 and msg.startswith(name + ":"), (rc, msg)


@pytest.mark.parametrize("fused,other", [(2, "ctn_dw_bwd_cln"), (3, "ctn_dw_bwd_gln2")])
def test_dw_bwd_refuses_the_forms_that_have_their_own_entry_point(fused, other):
    rc, msg = _dw_call("ctn_dw_bwd", fused=fused)
    assert rc == -1 and msg.startswith("ctn_dw_bwd:") and other in msg, (rc, msg)


@pytest.mark.parametrize("tag,nt,causal", [("gLN", "gLN", False), ("cLN", "cLN", True)])
def test_constructor_is_bitwise_the_reference_constructor(tag, nt, causal):
    g = load_golden("init_seed11_" + tag)
    N, L, B, H, P, X, R, C = [int(v) for v in g["cfg"]]
    torch.manual_seed(11)
    m = ctn.ConvTasNet(N, L, B, H, P, X, R, C, norm_type=nt, causal=causal)
    sd = m.state_dict()
    ref_keys = [k[2:] for k in g if k.startswith("p:")]
    assert list(sd.keys()) == ref_keys
    for k in ref_keys:
        assert np.array_equal(sd[k].numpy(), g["p:" + k]), k
    cfg = O.Config(N, L, B, H, P, X, R, C, norm_type=nt, causal=causal)
    assert [n for n, _ in m.named_parameters()] == list(O.param_shapes(cfg).keys())
    # D10: gamma/beta are xavier-initialised, PReLU slopes stay 0.25
    assert float(sd["separator.network.2.0.0.net.1.weight"]) == 0.25
    assert float(sd["separator.network.0.gamma"].std()) > 0.05


def test_paper_config_parameter_count():
    m = ctn.ConvTasNet(256, 20, 256, 512, 3, 8, 4, 2)
    ps = list(m.parameters())
    assert len(ps) == 294 and sum(p.numel() for p in ps) == 8710720


def test_serialize_and_load_round_trip(tmp_path):
    torch.manual_seed(0)
    m = ctn.ConvTasNet(16, 20, 8, 16, 3, 2, 1, 2, norm_type="cLN", causal=True, mask_nonlinear="softmax")
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    pkg = ctn.ConvTasNet.serialize(m, opt, 3, tr_loss=torch.zeros(4), cv_loss=torch.ones(4))
    assert sorted(pkg.keys()) == sorted(['N', 'L', 'B', 'H', 'P', 'X', 'R', 'C', 'norm_type', 'causal', 'mask_nonlinear',
                                         'state_dict', 'optim_dict', 'epoch', 'tr_loss', 'cv_loss'])
    g = load_golden("solver_traj")
    assert sorted(pkg.keys()) == sorted(str(k) for k in g["pkg_keys"])     # same package keys as the reference wrote
    path = str(tmp_path / "m.pth.tar")
    torch.save(pkg, path)
    m2 = ctn.ConvTasNet.load_model(path)
    assert m2.causal and m2.norm_type == "cLN" and m2.mask_nonlinear == "softmax"
    for (k1, v1), (k2, v2) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)


def test_reference_state_dict_loads():
    g = load_golden("model_tiny_cln_causal")
    N, L, B, H, P, X, R, C = [int(v) for v in g["cfg"]]
    m = ctn.ConvTasNet(N, L, B, H, P, X, R, C, norm_type="cLN", causal=True)
    m.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p:")})


def test_product_path_has_no_cpu_fallback():
    m = ctn.ConvTasNet(16, 20, 8, 16, 3, 2, 1, 2)
    with pytest.raises(ctn.CtnError):
        m(torch.randn(1, 400))
    with pytest.raises(ctn.CtnError):
        ctn.cal_loss(torch.randn(1, 2, 100), torch.randn(1, 2, 100), torch.tensor([100]))
    with pytest.raises(ValueError):
        ctn.ConvTasNet(16, 20, 8, 16, 3, 2, 1, 2, mask_nonlinear="sigmoid").separator.softmax_mask()


def test_missing_library_fails_loudly(monkeypatch):
    fresh = _lib._Lib()
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libctn_hip.so")
    with pytest.raises(ctn.CtnError, match="no CPU fallback"):
        fresh.load()


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "conv-tasnet_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "oracle" not in src.replace("# oracle", ""), fn


def test_halving_schedule_matches_reference_rule():
    s = _HalvingSchedule(True, True)
    seq = [5.0, 4.0, 4.5, 4.6, 4.7, 4.8, 4.1, 4.2, 4.3, 4.4, 4.5, 4.6, 4.7, 4.8]
    out = [s.update(v) for v in seq]
    # misses: 0,0,1,2,3(halve),4(halve),0,1,2,3(halve),4,5,6,7(stop)
    assert [h for h, _ in out] == [False, False, False, False, True, True, False, False, False, True, True, True, True, True]
    assert [st for _, st in out][-1] is True and not any(st for _, st in out[:-1])
    off = _HalvingSchedule(False, True)
    assert all(off.update(v) == (False, False) for v in [3, 4, 5, 6, 7, 8, 9, 10])


def test_overlap_and_add_reference_main_example_via_oracle():
    g = load_golden("ola_main_int")
    out = O.overlap_and_add(torch.from_numpy(g["signal"]).double(), int(g["step"]))
    assert np.array_equal(out.numpy().astype(np.int64), g["result"])
