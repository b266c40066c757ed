"""What the optional profiles record (bench.py's `stages` list and conv roofline): StageProfile's (name, flops, bytes, launches) of
the ten wrapped operations and ConvProfile's counters and shape keys, as literals recorded before the stage wrappers moved to the
definitions and conv()'s accounting into ConvProfile.record.

The CPU tests need neither a GPU nor a library: the first argument is a host tensor that reports is_cuda, torch.cuda.Event is a
stand-in, and the launch (ops._call), the device check and the stream lookup are stubbed -- the wrapped functions still validate their
arguments and allocate their results, which is all the work formulas read."""
import pytest
import torch

from aicovergen_amd import ops


class _OnDevice(torch.Tensor):
    """A host tensor that says it lives on the device (the profiles time nothing else)."""
    is_cuda = property(lambda self: True)


class _Event:
    def __init__(self, enable_timing=False):
        assert enable_timing

    def record(self):
        pass


def _dev(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_OnDevice)


@pytest.fixture
def no_launch(monkeypatch):
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    monkeypatch.setattr(ops, "_call", lambda name, *args: None)
    monkeypatch.setattr(ops, "_check", lambda *tensors: None)
    monkeypatch.setattr(ops, "_stream", lambda t: 0)


def _stage_calls():
    z = torch.zeros
    return {
        "stft": lambda: ops.stft(_dev(2, 4096), 512, 128, n_bins_out=200),
        "istft": lambda: ops.istft(_dev(2, 2, 257, 9), 512, 128, 1024),
        "linear_last": lambda: ops.linear_last(_dev(1, 2, 3, 16), z(24, 16), z(24), res=z(1, 2, 3, 24)),
        "tdf_pair": lambda: ops.tdf_pair(_dev(1, 2, 3, 32), z(4, 2, 8, 4), z(8), z(2), z(2), z(1, 512), z(32), z(2), z(2)),
        "dense_nt": lambda: ops.dense_nt(_dev(5, 16), z(24, 16), z(24), act=ops.ACT_SIGMOID),
        "attention": lambda: ops.attention(_dev(8, 40), z(8, 40), z(8, 40), 2),
        "sine_source": lambda: ops.sine_source(_dev(6), z(60), 10, 16000, 1.0, 0.0),
        "sine_source_window": lambda: ops.sine_source_window(_dev(6), z(60), 10, 16000, 1.0, 0.0, 7, 21),
        "layernorm_ct": lambda: ops.layernorm_ct(_dev(1, 4, 10), z(4), z(4), res=z(1, 4, 10)),
        "rownorm_act": lambda: ops.rownorm_act(_dev(3, 50), z(3), z(3), act=ops.ACT_GELU),
    }


# operation: (stage name, flops, bytes, launches, how its docstring begins)
STAGES = {
    "stft": ("stft", 0.0, 138368.0, 1, 'x: (n_sig, L) fp32.  Returns the complex spectro'),
    "istft": ("istft", 0.0, 45200.0, 1, 'spec: (n_sig, 2, n_bins_in, n_frames) (or (n_sig'),
    "linear_last": ("tdf_gemm_nt", 4608.0, 3072.0, 1, 'nn.Linear over the last axis of a contiguous (B,'),
    "tdf_pair": ("tdf_pair", 6144.0, 3584.0, 1, 'x + relu(bn2(relu(bn1(x W1^T + b1)) W2^T + b2)) '),
    "dense_nt": ("dense_gemm_nt", 3840.0, 2336.0, 1, 'act(x @ weight.T + bias) for a contiguous (rows,'),
    "attention": ("attention", 51200.0, 5120.0, 1, 'q, k, v: (C, T) channel-major (rows may be slice'),
    "sine_source": ("sine_source", 0.0, 504.0, 1, 'f0: (T,) Hz; noise: (T*upp,) N(0,1) draws -> har'),
    "sine_source_window": ("sine_source", 0.0, 192.0, 1, 'Samples first .. first + count - 1 of sine_sourc'),
    "layernorm_ct": ("layernorm", 0.0, 480.0, 1, 'LayerNorm over channels of contiguous (N, C, T);'),
    "rownorm_act": ("groupnorm_gelu", 0.0, 1200.0, 1, 'x: (rows, T), unit stride along T: per-row (x - '),
}


@pytest.mark.parametrize("op", list(_stage_calls()))
def test_stage_record(op, no_launch, monkeypatch):
    name, flops, nbytes, launches, _ = STAGES[op]
    monkeypatch.setattr(ops, "stage_profile", ops.StageProfile())
    _stage_calls()[op]()
    rec = ops.stage_profile.rec
    assert list(rec) == [name]
    assert (rec[name]["flops"], rec[name]["bytes"], rec[name]["launches"], len(rec[name]["events"])) == (flops, nbytes, launches, launches)


def test_both_sine_sources_share_a_stage(no_launch, monkeypatch):
    monkeypatch.setattr(ops, "stage_profile", ops.StageProfile())
    _stage_calls()["sine_source"]()
    _stage_calls()["sine_source_window"]()
    rec = ops.stage_profile.rec
    assert list(rec) == ["sine_source"] and rec["sine_source"]["launches"] == 2
    assert rec["sine_source"]["bytes"] == STAGES["sine_source"][2] + STAGES["sine_source_window"][2]


def test_dense_nt_is_counted_once_under_its_own_name(no_launch, monkeypatch):
    monkeypatch.setattr(ops, "stage_profile", ops.StageProfile())
    _stage_calls()["dense_nt"]()
    assert list(ops.stage_profile.rec) == ["dense_gemm_nt"] and ops.stage_profile.rec["dense_gemm_nt"]["launches"] == 1


@pytest.mark.parametrize("op", list(_stage_calls()))
def test_wrapped_functions_keep_name_and_docstring(op):
    fn = getattr(ops, op)
    assert fn.__name__ == op
    assert fn.__doc__.startswith(STAGES[op][4])


def test_nothing_is_timed_without_a_profile_or_off_the_device(no_launch, monkeypatch):
    class _NoEvent:
        def __init__(self, *a, **k):
            raise AssertionError("an event was created")

    monkeypatch.setattr(torch.cuda, "Event", _NoEvent)
    monkeypatch.setattr(ops, "stage_profile", None)
    monkeypatch.setattr(ops, "conv_profile", None)
    _stage_calls()["attention"]()
    _conv_launches(_dev)
    monkeypatch.setattr(ops, "stage_profile", ops.StageProfile())
    monkeypatch.setattr(ops, "conv_profile", ops.ConvProfile())
    ops.attention(torch.zeros(8, 40), torch.zeros(8, 40), torch.zeros(8, 40), 2)
    _conv_launches(torch.zeros)
    assert ops.stage_profile.rec == {} and ops.conv_profile.launches == 0 and ops.conv_profile.events == []


# ConvProfile over _conv_launches: launches, flops, flops_executed, bytes, shape keys with their flops
CONV_PROFILE = {
    "launches": 4,
    "flops": 9955328.0,
    "flops_executed": 6722218.666666666,
    "bytes": 395392.0,
    "shapes": [
        ("N1 C16>32 1x510 k1x3 s1,1 d1,1 g1", 1566720.0),
        ("N1 C8>32 4x64 k3x3 s1,1 d1,1 g1 wino", 1179648.0),
        ("N1 C8>48 8x64 k3x3 s1,1 d1,1 g1 wino2", 3538944.0),
        ("N1 C16>32 1x512 k1x7 s1,1 d1,3 g1 wino1d", 3670016.0),
    ],
}
CONV_PROFILE_MARKS = {   # ... with marks=True
    "launches": 6,
    "flops": 12046336.0,
    "flops_executed": 8813226.666666666,
    "bytes": 781568.0,
    "shapes": [
        ("N1 C16>32 1x510 k1x3 s1,1 d1,1 g1", 1566720.0),
        ("N1 C8>32 4x64 k3x3 s1,1 d1,1 g1 wino", 1179648.0),
        ("N1 C8>48 8x64 k3x3 s1,1 d1,1 g1 wino2", 3538944.0),
        ("N1 C16>32 1x512 k1x7 s1,1 d1,3 g1 wino1d", 3670016.0),
        ("N1 C16>32 1x510 k1x3 s1,1 d1,1 g1 res acc", 1566720.0),
        ("N1 C16>64 4x64 k1x1 s1,1 d1,1 g1 res shuf", 524288.0),
    ],
}

_CONV_KNOBS = dict(winograd=True, winograd_min_positions=1, winograd2d=True, winograd2d_code=0, winograd2d_waves=8, winograd2d_quads=False,
                   winograd2d_pairs=True, winograd1d=True, winograd1d_min_positions=1, gemm_tile=0, split_precision=False)


def _conv_launches(make, marks=False):
    """Direct, row form, two-dimensional form, dilated one-dimensional form (the base shapes of tests/test_conv_form.py); `marks`: then
    the epilogue marks of the shape key -- residual + accumulate on the direct form, the pixel-shuffle GEMM of a transposed convolution."""
    old = {k: getattr(ops, k) for k in _CONV_KNOBS}
    try:
        for k, v in _CONV_KNOBS.items():
            setattr(ops, k, v)
        dev = make(1).device
        pc = ops.PackedConv(torch.zeros(32, 16, 3), torch.zeros(32), padding=1, device=dev)
        ops.conv(make(1, 16, 510), pc)
        ops.conv(make(1, 8, 4, 64), ops.PackedConv(torch.zeros(32, 8, 3, 3), torch.zeros(32), padding=1, device=dev))
        ops.conv(make(1, 8, 8, 64), ops.PackedConv(torch.zeros(48, 8, 3, 3), torch.zeros(48), padding=1, device=dev), act=ops.ACT_RELU)
        ops.conv(make(1, 16, 512), ops.PackedConv(torch.zeros(32, 16, 7), torch.zeros(32), padding=9, dilation=3, device=dev))
        if marks:
            ops.conv(make(1, 16, 510), pc, res=make(1, 32, 510), out=make(1, 32, 510), accumulate=True)
            pt = ops.PackedConvTranspose(torch.zeros(16, 16, 2, 2), torch.zeros(16), stride=2, device=dev)
            ops.conv_transpose(make(1, 16, 4, 64), pt, mul=make(1, 16, 8, 128))
    finally:
        for k, v in old.items():
            setattr(ops, k, v)


def _profile_facts(prof):
    return {"launches": prof.launches, "flops": prof.flops, "flops_executed": prof.flops_executed, "bytes": prof.bytes, "shapes": prof.shapes}


def test_conv_profile_record(no_launch, monkeypatch):
    monkeypatch.setattr(ops, "conv_profile", ops.ConvProfile())
    _conv_launches(_dev)
    assert _profile_facts(ops.conv_profile) == CONV_PROFILE
    assert len(ops.conv_profile.events) == CONV_PROFILE["launches"] == 4
    monkeypatch.setattr(ops, "conv_profile", ops.ConvProfile())
    _conv_launches(_dev, marks=True)
    assert _profile_facts(ops.conv_profile) == CONV_PROFILE_MARKS


@pytest.mark.gpu
def test_conv_profile_on_the_device(monkeypatch):
    from conftest import _bind
    _bind("hip")
    monkeypatch.setattr(ops, "conv_profile", ops.ConvProfile())
    _conv_launches(lambda *shape: torch.zeros(*shape, device="cuda:0"))
    assert _profile_facts(ops.conv_profile) == CONV_PROFILE
    assert ops.conv_profile.summary()["launches"] == CONV_PROFILE["launches"] and len(ops.conv_profile.by_shape()) == len(set(k for k, _ in CONV_PROFILE["shapes"]))
