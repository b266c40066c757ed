"""What ops.conv hands to the library, pinned call by call: the aicg_conv_desc field by field, which weight image the pointer is, and
which of aicg_conv_forward / aicg_conv_forward_planned is called (with its plan_w).  Nothing here compares numbers (the parity tests do).

One base case per Winograd form, then one row per clause of that form's predicate, flipping that clause alone so that the form is lost.
CASES says, readably, what each row expects (entry point, aicg_conv_desc.wino, image); DESC holds the complete descriptor of every row.
Both are literals recorded from ops.conv as it stood when its body still derived all of this inline: a change to them is a change of
what the library is asked to do, never a re-recording.  PackedConv's packing (which images a layer carries, the lazily built ones) is
pinned the same way at the end."""
import pytest
import torch

from aicovergen_amd import ops

FIELDS = tuple(n for n, _ in ops.ConvDesc._fields_)

# every switch conv() and PackedConv read, at a known value (the forms are then enabled row by row)
KNOBS = dict(winograd=True, winograd_min_positions=1 << 60, winograd2d=False, winograd2d_code=0, winograd2d_waves=8, winograd2d_quads=False,
             winograd2d_pairs=True, winograd1d=True, winograd1d_min_positions=1 << 60, gemm_tile=0, split_precision=False, conv_profile=None)
ROWS = dict(winograd_min_positions=1)
W2D = dict(winograd_min_positions=1, winograd2d=True)
W1D = dict(winograd1d_min_positions=1)

FWD, PLANNED = "aicg_conv_forward", "aicg_conv_forward_planned"


def case(expect, knobs=None, ci=8, co=32, k=(3, 3), pad=1, dil=1, hw=(4, 64), **call):
    """expect: (entry point, aicg_conv_desc.wino, image name).  call: conv()'s keywords; res / out: True or how the operand is laid out
    (_tensor); x: how the input is laid out; f16 / pad_end: set on the layer."""
    return dict(expect=expect, knobs=knobs or {}, ci=ci, co=co, k=k, pad=pad, dil=dil, hw=hw, call=call)


def case1d(expect, knobs=W1D, ci=16, co=32, k=3, pad=1, dil=1, hw=512, **call):
    return case(expect, knobs, ci, co, k, pad, dil, hw, **call)


CASES = {
    # the row form F(2, 3): 8 -> 32 channels, 3 x 3, pad 1, a 4 x 64 map
    "rows": case((FWD, 1, "w_wino"), ROWS),
    "rows_res": case((FWD, 0, "w"), ROWS, res=True),
    "rows_accumulate": case((FWD, 0, "w"), ROWS, out=True, accumulate=True),
    "rows_pre_act": case((FWD, 0, "w"), ROWS, pre_act=ops.ACT_LRELU, pre_slope=0.1),
    "rows_out_scale": case((FWD, 0, "w"), ROWS, out_scale=0.5),
    "rows_gelu": case((FWD, 0, "w"), ROWS, act=ops.ACT_GELU),
    "rows_relu_keeps_the_form": case((FWD, 1, "w_wino"), ROWS, act=ops.ACT_RELU),
    "rows_odd_width": case((FWD, 0, "w"), ROWS, hw=(4, 63)),
    "rows_below_gate": case((FWD, 0, "w"), dict(winograd_min_positions=4 * 64 + 1)),
    "rows_at_gate": case((FWD, 1, "w_wino"), dict(winograd_min_positions=4 * 64)),
    # the two-dimensional form F(2 x 2, 3 x 3): 8 -> 48, an 8 x 64 map; a lost clause leaves the row form
    "w2d": case((FWD, 12, "wino2:pairs"), W2D, co=48, hw=(8, 64)),
    "w2d_dword": case((FWD, 2, "wino2:dword"), dict(W2D, winograd2d_pairs=False), co=48, hw=(8, 64)),
    "w2d_quads_4_waves": case((FWD, 5, "wino2:quads"), dict(W2D, winograd2d_quads=True, winograd2d_waves=4), co=48, hw=(8, 64)),
    "w2d_width_66": case((FWD, 1, "w_wino"), W2D, co=48, hw=(8, 66)),
    "w2d_x_one_float_in": case((FWD, 1, "w_wino"), W2D, co=48, hw=(8, 64), x="offset"),
    "w2d_channel_stride": case((FWD, 1, "w_wino"), W2D, co=48, hw=(8, 64), x="channel"),
    "w2d_32_out": case((FWD, 1, "w_wino"), W2D, co=32, hw=(8, 64)),
    "w2d_switched_off_after_packing": case((FWD, 1, "w_wino"), W2D, co=48, hw=(8, 64), late=dict(winograd2d=False)),
    # the one-dimensional form (csrc/conv_g1w.h): 16 -> 32, k = 3, pad 1, 512 positions
    "w1d": case1d((FWD, 8, "w_wino1")),
    "w1d_8_out": case1d((FWD, 0, "w"), co=8),
    "w1d_width_510": case1d((FWD, 0, "w"), hw=510),
    "w1d_below_gate": case1d((FWD, 0, "w"), dict(winograd1d_min_positions=513)),
    "w1d_plan_w_over_gate": case1d((PLANNED, 8, "w_wino1"), dict(winograd1d_min_positions=513), plan_w=1024),
    "w1d_plan_w_below_gate": case1d((PLANNED, 0, "w"), dict(winograd1d_min_positions=1025), plan_w=1024),
    "w1d_lrelu_keeps_the_form": case1d((FWD, 8, "w_wino1"), pre_act=ops.ACT_LRELU, pre_slope=0.1, res=True),
    "w1d_gelu_pre_act": case1d((FWD, 0, "w"), pre_act=ops.ACT_GELU),
    "w1d_pre_slope": case1d((FWD, 0, "w"), pre_act=ops.ACT_LRELU, pre_slope=1.5),
    "w1d_out_len": case1d((FWD, 0, "w"), out_len=508),
    "w1d_x_misaligned": case1d((FWD, 0, "w"), x="offset"),
    "w1d_out_misaligned": case1d((FWD, 0, "w"), out="offset"),
    "w1d_res_misaligned": case1d((FWD, 0, "w"), res="offset"),
    "w1d_x_channel_stride": case1d((FWD, 0, "w"), x="channel"),
    "w1d_switched_off_after_packing": case1d((FWD, 0, "w"), late=dict(winograd1d=False)),
    "w1d_k7_d3": case1d((FWD, 8, "w_wino1"), k=7, pad=9, dil=3),
    "w1d_k5_d1": case1d((FWD, 8, "w_wino1"), k=5, pad=2),
    "w1d_k5_d3_has_no_image": case1d((FWD, 0, "w"), k=5, pad=6, dil=3),
    "w1d_2d_input_of_one_row": case1d((FWD, 0, "w"), x="as4d"),
    # what else reaches the descriptor
    "split_layer": case1d((FWD, 0, "w"), dict(split_precision=True), hw=300),
    "f16_layer": case1d((FWD, 8, "w_wino1"), f16=True),
    "padding_end": case1d((FWD, 0, "w"), ci=4, co=8, k=4, pad=1, hw=64, pad_end=2),
    "transpose_shuffle_mul": case((FWD, 0, "w"), ROWS, ci=16, co=16, hw=(4, 64), up="mul"),
    "transpose_shuffle_add": case((FWD, 0, "w"), ROWS, ci=16, co=16, hw=(4, 64), up="add"),
    "gemm_tile": case1d((FWD, 0, "w"), dict(gemm_tile=1), k=1, pad=0, hw=128),
    "bias_override_and_res_before_act": case((FWD, 0, "w"), ROWS, res=True, res_before_act=True, act=ops.ACT_RELU, bias=True),
}

# aicg_conv_desc of every row, in FIELDS order
DESC = {
    "rows": (1, 8, 4, 64, 32, 4, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 2048, 256, 64, 8192, 256, 64, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 1, 0),
    "rows_res": (1, 8, 4, 64, 32, 4, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 2048, 256, 64, 8192, 256, 64, 8192, 256, 64, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "rows_accumulate": (1, 8, 4, 64, 32, 4, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 2048, 256, 64, 8192, 256, 64, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 1, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "rows_pre_act": (1, 8, 4, 64, 32, 4, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 2048, 256, 64, 8192, 256, 64, 0, 0, 0, 2, 0.10000000149011612, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "rows_out_scale": (1, 8, 4, 64, 32, 4, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 2048, 256, 64, 8192, 256, 64, 0, 0, 0, 0, 0.0, 0, 0.0, 0.5, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "rows_gelu": (1, 8, 4, 64, 32, 4, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 2048, 256, 64, 8192, 256, 64, 0, 0, 0, 0, 0.0, 3, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "rows_relu_keeps_the_form": (1, 8, 4, 64, 32, 4, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 2048, 256, 64, 8192, 256, 64, 0, 0, 0, 0, 0.0, 1, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 1, 0),
    "rows_odd_width": (1, 8, 4, 63, 32, 4, 63, 3, 3, 1, 1, 1, 1, 1, 1, 1, 2016, 252, 63, 8064, 252, 63, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "rows_below_gate": (1, 8, 4, 64, 32, 4, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 2048, 256, 64, 8192, 256, 64, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "rows_at_gate": (1, 8, 4, 64, 32, 4, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 2048, 256, 64, 8192, 256, 64, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 1, 0),
    "w2d": (1, 8, 8, 64, 48, 8, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 4096, 512, 64, 24576, 512, 64, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 12, 0),
    "w2d_dword": (1, 8, 8, 64, 48, 8, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 4096, 512, 64, 24576, 512, 64, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 2, 0),
    "w2d_quads_4_waves": (1, 8, 8, 64, 48, 8, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 4096, 512, 64, 24576, 512, 64, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 5, 0),
    "w2d_width_66": (1, 8, 8, 66, 48, 8, 66, 3, 3, 1, 1, 1, 1, 1, 1, 1, 4224, 528, 66, 25344, 528, 66, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 1, 0),
    "w2d_x_one_float_in": (1, 8, 8, 64, 48, 8, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 4096, 512, 64, 24576, 512, 64, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 1, 0),
    "w2d_channel_stride": (1, 8, 8, 64, 48, 8, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 4112, 514, 64, 24576, 512, 64, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 1, 0),
    "w2d_32_out": (1, 8, 8, 64, 32, 8, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 4096, 512, 64, 16384, 512, 64, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 1, 0),
    "w2d_switched_off_after_packing": (1, 8, 8, 64, 48, 8, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 4096, 512, 64, 24576, 512, 64, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 1, 0),
    "w1d": (1, 16, 1, 512, 32, 1, 512, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8192, 512, 512, 16384, 512, 512, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 8, 0),
    "w1d_8_out": (1, 16, 1, 512, 8, 1, 512, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8192, 512, 512, 4096, 512, 512, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "w1d_width_510": (1, 16, 1, 510, 32, 1, 510, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8160, 510, 510, 16320, 510, 510, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "w1d_below_gate": (1, 16, 1, 512, 32, 1, 512, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8192, 512, 512, 16384, 512, 512, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "w1d_plan_w_over_gate": (1, 16, 1, 512, 32, 1, 512, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8192, 512, 512, 16384, 512, 512, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 8, 0),
    "w1d_plan_w_below_gate": (1, 16, 1, 512, 32, 1, 512, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8192, 512, 512, 16384, 512, 512, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "w1d_lrelu_keeps_the_form": (1, 16, 1, 512, 32, 1, 512, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8192, 512, 512, 16384, 512, 512, 16384, 512, 512, 2, 0.10000000149011612, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 8, 0),
    "w1d_gelu_pre_act": (1, 16, 1, 512, 32, 1, 512, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8192, 512, 512, 16384, 512, 512, 0, 0, 0, 3, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "w1d_pre_slope": (1, 16, 1, 512, 32, 1, 512, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8192, 512, 512, 16384, 512, 512, 0, 0, 0, 2, 1.5, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "w1d_out_len": (1, 16, 1, 512, 32, 1, 508, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8192, 512, 512, 16256, 508, 508, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "w1d_x_misaligned": (1, 16, 1, 512, 32, 1, 512, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8192, 512, 512, 16384, 512, 512, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "w1d_out_misaligned": (1, 16, 1, 512, 32, 1, 512, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8192, 512, 512, 16384, 512, 512, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "w1d_res_misaligned": (1, 16, 1, 512, 32, 1, 512, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8192, 512, 512, 16384, 512, 512, 16384, 512, 512, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "w1d_x_channel_stride": (1, 16, 1, 512, 32, 1, 512, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8224, 514, 512, 16384, 512, 512, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "w1d_switched_off_after_packing": (1, 16, 1, 512, 32, 1, 512, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8192, 512, 512, 16384, 512, 512, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "w1d_k7_d3": (1, 16, 1, 512, 32, 1, 512, 1, 7, 1, 1, 0, 9, 1, 3, 1, 8192, 512, 512, 16384, 512, 512, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 8, 0),
    "w1d_k5_d1": (1, 16, 1, 512, 32, 1, 512, 1, 5, 1, 1, 0, 2, 1, 1, 1, 8192, 512, 512, 16384, 512, 512, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 8, 0),
    "w1d_k5_d3_has_no_image": (1, 16, 1, 512, 32, 1, 512, 1, 5, 1, 1, 0, 6, 1, 3, 1, 8192, 512, 512, 16384, 512, 512, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "w1d_2d_input_of_one_row": (1, 16, 1, 512, 32, 1, 512, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8192, 512, 512, 16384, 512, 512, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 0),
    "split_layer": (1, 16, 1, 300, 32, 1, 300, 1, 3, 1, 1, 0, 1, 1, 1, 1, 4800, 300, 300, 9600, 300, 300, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 1, 0, 0),
    "f16_layer": (1, 16, 1, 512, 32, 1, 512, 1, 3, 1, 1, 0, 1, 1, 1, 1, 8192, 512, 512, 16384, 512, 512, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 2, 8, 0),
    "padding_end": (1, 4, 1, 64, 8, 1, 64, 1, 4, 1, 1, 0, 1, 1, 1, 1, 256, 64, 64, 512, 64, 64, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, 0, 2, 0, 0, 1, 0, 0, 0),
    "transpose_shuffle_mul": (1, 16, 4, 64, 64, 4, 64, 1, 1, 1, 1, 0, 0, 1, 1, 1, 4096, 256, 64, 16384, 1024, 128, 16384, 1024, 128, 0, 0.0, 1, 0.0, 1.0, 0, 0, -1, -1, 2, 1, 1, 0, 0, 0),
    "transpose_shuffle_add": (1, 16, 4, 64, 64, 4, 64, 1, 1, 1, 1, 0, 0, 1, 1, 1, 4096, 256, 64, 16384, 1024, 128, 16384, 1024, 128, 0, 0.0, 1, 0.0, 1.0, 0, 0, -1, -1, 2, 0, 1, 0, 0, 0),
    "gemm_tile": (1, 16, 1, 128, 32, 1, 128, 1, 1, 1, 1, 0, 0, 1, 1, 1, 2048, 128, 128, 4096, 128, 128, 0, 0, 0, 0, 0.0, 0, 0.0, 1.0, 0, 0, -1, -1, 0, 0, 1, 0, 0, 1),
    "bias_override_and_res_before_act": (1, 8, 4, 64, 32, 4, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1, 2048, 256, 64, 8192, 256, 64, 8192, 256, 64, 0, 0.0, 1, 0.0, 1.0, 0, 1, -1, -1, 0, 0, 1, 0, 0, 0),
}


def _tensor(shape, how, dev):
    """how: True / None: contiguous; "offset": a view starting one float into its storage; "channel": a channel stride of two
    floats more than a channel; "as4d" (1-D shapes): the (N, C, 1, W) form."""
    numel = 1
    for s in shape:
        numel *= s
    if how == "offset":
        return dev.t(torch.randn(numel + 1))[1:].view(shape)
    if how == "channel":
        per = numel // (shape[0] * shape[1])
        t = dev.t(torch.randn(shape[0], shape[1], per + 2))[:, :, :per]
        return t if len(shape) == 3 else t.unflatten(2, shape[2:])
    t = dev.t(torch.randn(shape))
    return t.unsqueeze(2) if how == "as4d" else t


def _image_name(pc, ptr):
    named = [("w", pc.w), ("w_wino", pc.w_wino), ("w_wino1", pc.w_wino1)]
    if pc.w_wino2 is not None:
        named += [("wino2:" + kind, pc.wino2_image(kind)) for kind in ("dword", "pairs", "quads")]
    hits = [name for name, t in named if t is not None and t.data_ptr() == ptr]
    assert len(hits) == 1, hits
    return hits[0]


def observe(name, dev, monkeypatch):
    """Run one row; returns ((entry point, wino, image name), plan_w, descriptor fields)."""
    c = CASES[name]
    call = dict(c["call"])
    torch.manual_seed(0)
    for k, v in dict(KNOBS, **c["knobs"]).items():
        monkeypatch.setattr(ops, k, v)
    seen = []
    real = ops._call

    def spy(fn, *args):
        if fn in (FWD, PLANNED):
            d = ops.ConvDesc.from_address(args[0])
            seen.append((fn, tuple(getattr(d, f) for f in FIELDS), args[2], args[6] if fn == PLANNED else None))
        return real(fn, *args)

    monkeypatch.setattr(ops, "_call", spy)
    n, ci, co, k, hw = 1, c["ci"], c["co"], c["k"], c["hw"]
    up = call.pop("up", None)
    if up:
        pt = ops.PackedConvTranspose(torch.randn(ci, co, 2, 2) * 0.2, torch.randn(co), stride=2, device=dev.device)
        pc = pt.gemm
        skip = dev.t(torch.randn(n, co, 2 * hw[0], 2 * hw[1]))
        ops.conv_transpose(_tensor((n, ci) + hw, None, dev), pt, act=ops.ACT_RELU, **{up: skip})
    else:
        one_d = isinstance(k, int)
        w = (torch.randn(co, ci, k) if one_d else torch.randn(co, ci, *k)) * 0.1
        pc = ops.PackedConv(w, torch.randn(co), padding=c["pad"], dilation=c["dil"], padding_end=call.pop("pad_end", None), device=dev.device)
        pc.f16 = bool(call.pop("f16", False))
        for kk, v in call.pop("late", {}).items():
            monkeypatch.setattr(ops, kk, v)
        x = _tensor((n, ci, hw) if one_d else (n, ci) + hw, call.pop("x", None), dev)
        ho, wo = pc.out_hw(1 if one_d else hw[0], hw if one_d else hw[1])
        oshape = (n, co, call.get("out_len", wo)) if one_d else (n, co, ho, wo)
        if x.dim() == 4 and one_d:
            oshape = (n, co, 1, oshape[2])
        for key in ("res", "out"):
            if call.get(key):
                call[key] = _tensor(oshape, call[key], dev)
        if call.get("bias"):
            call["bias"] = dev.t(torch.randn(co))
        ops.conv(x, pc, **call)
    dev.sync()
    assert len(seen) == 1, seen
    fn, fields, w_ptr, plan_w = seen[0]
    return (fn, fields[FIELDS.index("wino")], _image_name(pc, w_ptr)), plan_w, fields


@pytest.mark.parametrize("name", list(CASES))
def test_descriptor_image_and_entry_point(name, dev, monkeypatch):
    got, plan_w, fields = observe(name, dev, monkeypatch)
    assert got == CASES[name]["expect"]
    assert plan_w == CASES[name]["call"].get("plan_w")
    assert fields == DESC[name], [(f, a, b) for f, a, b in zip(FIELDS, fields, DESC[name]) if a != b]


def test_precision_codes(dev, monkeypatch):
    """aicg_conv_desc.split: 1 for a layer packed under split precision, 2 for one marked for fp16 operands, 0 otherwise."""
    split = FIELDS.index("split")
    assert observe("split_layer", dev, monkeypatch)[2][split] == 1
    assert observe("f16_layer", dev, monkeypatch)[2][split] == 2
    assert observe("w1d", dev, monkeypatch)[2][split] == 0


def _layer(kind, dev):
    torch.manual_seed(0)
    if kind in ("rows", "w2d"):
        co = 48 if kind == "w2d" else 32
        return ops.PackedConv(torch.randn(co, 8, 3, 3), torch.randn(co), padding=1, device=dev.device)
    return ops.PackedConv(torch.randn(32, 16, 3), torch.randn(32), padding=1, device=dev.device)


# layer: knobs while packing, under fp32_layers(), then (w_wino, w_wino1, w_wino2 exist, conv_h_supported())
PACKING = {
    "rows": (ROWS, False, (True, False, False, False)),
    "w2d": (W2D, False, (True, False, True, False)),
    "w1d": (W1D, False, (False, True, False, True)),
    "w1d_split": (dict(split_precision=True), False, (False, False, False, False)),
    "w2d_fp32_layers": (W2D, True, (False, False, False, False)),
    "w1d_fp32_layers": (W1D, True, (False, False, False, False)),
}


@pytest.mark.parametrize("name", list(PACKING))
def test_packed_images(name, dev, monkeypatch):
    knobs, fp32, expect = PACKING[name]
    for k, v in dict(KNOBS, **knobs).items():
        monkeypatch.setattr(ops, k, v)
    if fp32:
        with ops.fp32_layers():
            pc = _layer(name.split("_")[0], dev)
    else:
        pc = _layer(name.split("_")[0], dev)
    assert (pc.w_wino is not None, pc.w_wino1 is not None, pc.w_wino2 is not None, pc.conv_h_supported()) == expect
    assert pc.fp32_only == fp32 and pc.split == bool(knobs.get("split_precision")) and pc.f16 is False


def test_lazy_images_are_built_once(dev, monkeypatch):
    """Only the routed F(2 x 2, 3 x 3) image exists after packing; the other layouts and the fp16 image are built on first use, once."""
    for k, v in dict(KNOBS, **W2D).items():
        monkeypatch.setattr(ops, k, v)
    built = []
    real = ops.winograd2d_image
    monkeypatch.setattr(ops, "winograd2d_image", lambda w, quads=False, pairs=False: built.append((quads, pairs)) or real(w, quads=quads, pairs=pairs))
    pc = _layer("w2d", dev)
    assert built == [(False, True)] and pc.w_wino2 is pc.wino2_image("pairs")
    q = pc.wino2_image("quads")
    assert pc.wino2_image("quads") is q and built == [(False, True), (True, False)]
    assert q.shape == pc.w_wino2.shape == (48 * 8 * 16,) and q.data_ptr() != pc.w_wino2.data_ptr()
    assert built == [(False, True), (True, False)]
    h = _layer("w1d", dev)
    img = h.conv_h_image()
    assert h.conv_h_image() is img
    assert img.dtype == torch.float16 and tuple(img.shape) == (1, 2, 3, 2, 32, 4) and img.device.type == dev.device.type
    with pytest.raises(AssertionError):
        pc.conv_h_image()
