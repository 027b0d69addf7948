"""No GPU: the SGD / Adam+L2 optimiser entry points of the C ABI and the host-side checks of FlatSGD, FlatAdam and train()."""
import subprocess

import pytest
import torch

import conv_tasnet_amd as ctn
from conv_tasnet_amd import _lib
from conv_tasnet_amd.optim import FlatAdam, FlatSGD

NEW = ("ctn_clip_sgd_step", "ctn_clip_adam_l2_step")
# fake device addresses: every call below is rejected by an argument check before any launch, so none is dereferenced
A, B, C, WS = 0x10000, 0x20000, 0x30000, 0x40000


def test_header_declares_and_library_exports_the_new_optimiser_steps():
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos and protos[name][0] is _lib.ctypes.c_int
    assert protos["ctn_clip_sgd_step"][2] == ["params", "grads", "momentum_buf", "n", "grad_scale", "max_norm", "lr",
                                              "momentum", "dampening", "weight_decay", "nesterov", "first_step",
                                              "total_norm_out", "workspace", "stream"]
    assert protos["ctn_clip_adam_l2_step"][2] == protos["ctn_clip_adam_step"][2][:12] + ["weight_decay"] + \
        protos["ctn_clip_adam_step"][2][12:]
    out = subprocess.run(["nm", "-D", "--defined-only", ctn.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW) <= exported


def _sgd(params=A, grads=B, buf=C, n=16, momentum=0.9, dampening=0.0, nesterov=0, ws=WS):
    return ctn.lib.ctn_clip_sgd_step(params, grads, buf, n, 1.0, 5.0, 0.1, momentum, dampening, 1e-4, nesterov, 1, 0, ws, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(params=0), b"null"),
    (dict(grads=0), b"null"),
    (dict(ws=0), b"null"),
    (dict(buf=0), b"momentum_buf"),
    (dict(n=0), b"bad sizes"),
    (dict(n=-4), b"bad sizes"),
    (dict(grads=B + 4), b"aligned"),
    (dict(params=A + 8), b"aligned"),
    (dict(buf=C + 4), b"aligned"),
    (dict(nesterov=1, dampening=0.1), b"nesterov"),
    (dict(nesterov=1, momentum=0.0, buf=0), b"nesterov"),
])
def test_sgd_step_rejects_bad_arguments_before_any_launch(kw, msg):
    assert _sgd(**kw) == -1
    assert msg in ctn.lib.ctn_last_error()


def _adam_l2(params=A, grads=B, m=C, v=C + 0x10000, n=16, step=1, ws=WS):
    return ctn.lib.ctn_clip_adam_l2_step(params, grads, m, v, n, 1.0, 5.0, 1e-3, 0.9, 0.999, 1e-8, step, 1e-4, 0, ws, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(params=0), b"null"),
    (dict(m=0), b"null"),
    (dict(v=0), b"null"),
    (dict(ws=0), b"null"),
    (dict(n=0), b"bad sizes"),
    (dict(step=0), b"bad sizes"),
    (dict(grads=B + 4), b"aligned"),
    (dict(v=C + 0x10000 + 12), b"aligned"),
])
def test_adam_l2_step_rejects_bad_arguments_before_any_launch(kw, msg):
    assert _adam_l2(**kw) == -1
    assert msg in ctn.lib.ctn_last_error()


def test_bad_optimiser_arguments_raise_through_lib_call():
    with pytest.raises(ctn.CtnError, match="momentum_buf"):
        ctn.lib.call("ctn_clip_sgd_step", A, B, 0, 16, 1.0, 5.0, 0.1, 0.9, 0.0, 0.0, 0, 1, 0, WS, None)


def _cpu_params():
    return [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]


@pytest.mark.parametrize("kw,msg", [
    (dict(lr=-0.1), "Invalid learning rate"),
    (dict(momentum=-0.5), "Invalid momentum value"),
    (dict(weight_decay=-1e-4), "Invalid weight_decay value"),
    (dict(nesterov=True), "Nesterov momentum requires a momentum and zero dampening"),
    (dict(nesterov=True, momentum=0.9, dampening=0.1), "Nesterov momentum requires a momentum and zero dampening"),
    (dict(maximize=True), "maximize"),
])
def test_flat_sgd_validates_like_torch_before_touching_the_device(kw, msg):
    # CPU parameters: without the checks up front the constructor would fail on the device instead (CtnError)
    with pytest.raises(ValueError, match=msg):
        FlatSGD(_cpu_params(), **dict(dict(lr=0.1), **kw))
    if "maximize" not in kw:                        # torch.optim.SGD rejects the same values
        with pytest.raises(ValueError, match=msg):
            torch.optim.SGD(_cpu_params(), **dict(dict(lr=0.1), **kw))


@pytest.mark.parametrize("kw,msg", [
    (dict(lr=-1e-3), "Invalid learning rate"),
    (dict(eps=-1.0), "Invalid epsilon value"),
    (dict(betas=(1.0, 0.999)), "Invalid beta parameter at index 0"),
    (dict(betas=(0.9, -0.1)), "Invalid beta parameter at index 1"),
    (dict(weight_decay=-1e-4), "Invalid weight_decay value"),
    (dict(amsgrad=True), "amsgrad"),
    (dict(decoupled_weight_decay=True), "decoupled_weight_decay"),
])
def test_flat_adam_validates_before_touching_the_device(kw, msg):
    with pytest.raises(ValueError, match=msg):
        FlatAdam(_cpu_params(), **kw)


def test_flat_optimisers_with_valid_settings_still_need_the_gpu():
    for opt in (lambda ps: FlatSGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True),
                lambda ps: FlatAdam(ps, lr=1e-3, weight_decay=1e-4)):
        with pytest.raises(ctn.CtnError, match="GPU"):
            opt(_cpu_params())


def test_train_rejects_an_unknown_optimizer_like_the_reference(capsys, tmp_path):
    from conv_tasnet_amd.train import train
    out = train({"tr_loader": [], "cv_loader": []}, 1, "final.pth.tar", save_folder=str(tmp_path),
                optimizer_type="rmsprop")
    assert out is None
    assert "Not support optimizer" in capsys.readouterr().out
