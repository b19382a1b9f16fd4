"""ctypes binding of libsomi_hip.so (the C ABI declared in include/somi_hip.h).

The library is the product; this module only loads it, declares argument types and turns return
codes into exceptions.  There is no fallback: if the shared library is missing or an entry point
fails, a RuntimeError is raised (a reference-side `AT_ASSERTM` surfaces as RuntimeError too,
models/ops_dcnv3/src/cuda/dcnv3_cuda.cu:29-53).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SOMI_HIP_LIB') or os.path.join(os.path.dirname(_HERE), 'lib', 'libsomi_hip.so')   # override: kernel experiments

ABI_VERSION = 15         # SOMI_ABI_VERSION of include/somi_hip.h this binding was written against
c_f32p = C.c_void_p      # device pointers travel as integers
c_stream = C.c_void_p


class ConvDesc(C.Structure):
    """struct somi_conv_desc (include/somi_hip.h)."""
    _fields_ = [(n, C.c_void_p) for n in ('x', 'w', 'bias', 'post_scale', 'post_shift', 'residual', 'a_chan_scale',
                                          'a_pix_scale', 'y')] + \
               [(n, C.c_int32) for n in ('B', 'H', 'W', 'Cin', 'x_cs', 'x_coff', 'Ho', 'Wo', 'Cout', 'y_cs', 'y_coff',
                                         'kh', 'kw', 'stride', 'pad', 'dil', 'res_cs', 'res_coff', 'act', 'per_sample_w')] + \
               [('res2_cs', C.c_int32), ('res2_coff', C.c_int32), ('workspace', C.c_void_p), ('workspace_bytes', C.c_uint64),
                ('residual2', C.c_void_p), ('stat_sum', C.c_void_p), ('stat_sumsq', C.c_void_p), ('stat_pivot', C.c_void_p), ('prec', C.c_int32)]


class LossDesc(C.Structure):
    """struct somi_loss_desc (include/somi_hip.h)."""
    _fields_ = [('p', C.c_void_p * 4), ('grad', C.c_void_p * 4), ('ny', C.c_int32 * 4), ('nx', C.c_int32 * 4),
                ('nl', C.c_int32), ('na', C.c_int32), ('nc', C.c_int32), ('B', C.c_int32), ('nt', C.c_int32),
                ('targets', C.c_void_p), ('anchors', C.c_void_p), ('balance', C.c_float * 4),
                ('box_gain', C.c_float), ('obj_gain', C.c_float), ('cls_gain', C.c_float), ('cls_pw', C.c_float),
                ('obj_pw', C.c_float), ('anchor_t', C.c_float), ('cp', C.c_float), ('cn', C.c_float), ('gr', C.c_float),
                ('fl_gamma', C.c_float), ('slide', C.c_int32), ('nwd_ratio', C.c_float), ('nwd_constant', C.c_float)]


class LossLevel(C.Structure):
    """struct somi_loss_level (include/somi_hip.h): the fifth detection level of somi_yolo_loss5_f32."""
    _fields_ = [('p', C.c_void_p), ('grad', C.c_void_p), ('ny', C.c_int32), ('nx', C.c_int32), ('balance', C.c_float)]


class LossBoxRule(C.Structure):
    """struct somi_loss_box_rule (include/somi_hip.h): which box-regression rule the loss scores matched boxes with."""
    _fields_ = [('kind', C.c_int32), ('focal', C.c_int32), ('inner', C.c_int32), ('wiou_scaled', C.c_int32),
                ('alpha', C.c_float), ('gamma', C.c_float), ('inner_ratio', C.c_float), ('shape_scale', C.c_float),
                ('wiou_mean', C.c_void_p), ('wiou_train', C.c_int32)]


class Slice(C.Structure):
    """struct somi_slice (include/somi_hip.h): a channel slice as one argument."""
    _fields_ = [('p', C.c_void_p), ('cs', C.c_int32), ('coff', C.c_int32)]


class AsffDesc(C.Structure):
    """struct somi_asff_desc (include/somi_hip.h)."""
    _fields_ = [('r', Slice * 3), ('v', Slice * 3), ('r_up', C.c_int32 * 3), ('v_up', C.c_int32 * 3), ('w', C.c_void_p), ('bias', C.c_void_p),
                ('out', Slice), ('p', C.c_void_p), ('dr', Slice * 3), ('dv', Slice * 3), ('dr_accumulate', C.c_int32 * 3),
                ('B', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('C', C.c_int32), ('dw', C.c_void_p), ('db', C.c_void_p),
                ('workspace', C.c_void_p), ('workspace_floats', C.c_uint64)]


class CoordAttDesc(C.Structure):
    """struct somi_coordatt_desc (include/somi_hip.h)."""
    _fields_ = [('x', Slice), ('y', Slice), ('res', Slice), ('pool', Slice), ('a_h', Slice), ('a_w', Slice), ('a_h_rows', C.c_int32),
                ('a_w_rows', C.c_int32), ('r_h', Slice), ('r_w', Slice), ('r_h_rows', C.c_int32), ('r_w_rows', C.c_int32), ('dx', Slice),
                ('accumulate', C.c_int32), ('B', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('C', C.c_int32), ('workspace', C.c_void_p),
                ('workspace_floats', C.c_uint64)]


class EmaDesc(C.Structure):
    """struct somi_ema_desc (include/somi_hip.h)."""
    _fields_ = [('x', Slice), ('x2', Slice), ('sg', Slice), ('y', Slice), ('res', Slice), ('dx', Slice), ('dw', Slice), ('dsg', Slice),
                ('gamma', C.c_void_p), ('beta', C.c_void_p), ('stats', C.c_void_p), ('vec', C.c_void_p), ('sums', C.c_void_p),
                ('bvec', C.c_void_p), ('dgamma', C.c_void_p), ('dbeta', C.c_void_p), ('eps', C.c_float), ('factor', C.c_int32),
                ('accumulate', C.c_int32), ('B', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('C', C.c_int32), ('workspace', C.c_void_p),
                ('workspace_floats', C.c_uint64)]


class AcmixDesc(C.Structure):
    """struct somi_acmix_desc (include/somi_hip.h)."""
    _fields_ = [(n, Slice) for n in ('q', 'k', 'v', 'mix', 'out', 'lse', 'aux', 'dq', 'dk', 'dv')] + \
               [(n, C.c_void_p) for n in ('wp', 'rate1', 'rate2', 'weff', 'bias', 'dwp', 'drates', 'dweff', 'dbias')] + \
               [('accumulate', C.c_int32), ('B', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('C', C.c_int32), ('workspace', C.c_void_p),
                ('workspace_floats', C.c_uint64)]


class CpcaStripDesc(C.Structure):
    """struct somi_cpca_strip_desc (include/somi_hip.h)."""
    _fields_ = [('src', Slice * 4), ('dst', Slice * 3), ('w', C.c_void_p * 3), ('bias', C.c_void_p * 3), ('taps', C.c_int32 * 3),
                ('axis', C.c_int32), ('flip', C.c_int32), ('accumulate', C.c_int32), ('B', C.c_int32), ('H', C.c_int32), ('W', C.c_int32),
                ('C', C.c_int32)]


class CpcaWgradDesc(C.Structure):
    """struct somi_cpca_wgrad_desc (include/somi_hip.h)."""
    _fields_ = [('u', Slice), ('t', Slice * 3), ('ds', Slice), ('dt', Slice * 3), ('dw_h', C.c_void_p * 3), ('dw_v', C.c_void_p * 3),
                ('db_h', C.c_void_p * 3), ('db_v', C.c_void_p * 3), ('taps', C.c_int32 * 3), ('accumulate', C.c_int32), ('B', C.c_int32),
                ('H', C.c_int32), ('W', C.c_int32), ('C', C.c_int32), ('workspace', C.c_void_p), ('workspace_floats', C.c_uint64)]


class SimamDesc(C.Structure):
    """struct somi_simam_desc (include/somi_hip.h)."""
    _fields_ = [('x', Slice), ('y', Slice), ('dx', Slice), ('stats', C.c_void_p), ('sums', C.c_void_p), ('B', C.c_int32), ('H', C.c_int32),
                ('W', C.c_int32), ('C', C.c_int32), ('ny', C.c_int32), ('nx', C.c_int32), ('step_y', C.c_int32), ('step_x', C.c_int32),
                ('len_y', C.c_int32), ('len_x', C.c_int32), ('stretch_last', C.c_int32), ('add_input', C.c_int32), ('accumulate', C.c_int32),
                ('n', C.c_float), ('lam', C.c_float), ('workspace', C.c_void_p), ('workspace_floats', C.c_uint64)]


class ZoomcatDesc(C.Structure):
    """struct somi_zoomcat_desc (include/somi_hip.h)."""
    _fields_ = [('l', Slice), ('m', Slice), ('s', Slice), ('out', Slice), ('codes', C.c_void_p), ('B', C.c_int32), ('H', C.c_int32),
                ('W', C.c_int32), ('Cl', C.c_int32), ('Cm', C.c_int32), ('Cs', C.c_int32), ('accumulate', C.c_int32 * 3)]


class ScalseqDesc(C.Structure):
    """struct somi_scalseq_desc (include/somi_hip.h)."""
    _fields_ = [('u3', Slice), ('u4', Slice), ('u5', Slice), ('out', Slice), ('g3', Slice), ('g4', Slice), ('g5', Slice), ('codes', C.c_void_p),
                ('gamma', C.c_void_p), ('beta', C.c_void_p), ('mean', C.c_void_p), ('rstd', C.c_void_p), ('scale', C.c_void_p),
                ('shift', C.c_void_p), ('running_mean', C.c_void_p), ('running_var', C.c_void_p), ('sums', C.c_void_p), ('dgamma', C.c_void_p),
                ('dbeta', C.c_void_p), ('B', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('C', C.c_int32), ('eps', C.c_float),
                ('momentum', C.c_float), ('workspace', C.c_void_p), ('workspace_floats', C.c_uint64)]


class AsfAttDesc(C.Structure):
    """struct somi_asfatt_desc (include/somi_hip.h)."""
    _fields_ = [('x1', Slice), ('x2', Slice), ('t', Slice), ('pool', Slice), ('dx1', Slice), ('gate', C.c_void_p), ('ds', C.c_void_p),
                ('davg', C.c_void_p), ('B', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('C', C.c_int32), ('accumulate', C.c_int32),
                ('workspace', C.c_void_p), ('workspace_floats', C.c_uint64)]


class AugSource(C.Structure):
    """struct somi_aug_source (include/somi_hip.h)."""
    _fields_ = [('pixels', C.c_void_p), ('h', C.c_int32), ('w', C.c_int32), ('x1', C.c_int32), ('y1', C.c_int32),
                ('x2', C.c_int32), ('y2', C.c_int32), ('dx', C.c_int32), ('dy', C.c_int32)]


class AugCanvas(C.Structure):
    """struct somi_aug_canvas."""
    _fields_ = [('src', AugSource * 4), ('nsrc', C.c_int32), ('height', C.c_int32), ('width', C.c_int32), ('warp', C.c_int32),
                ('minv', C.c_double * 6)]


class AugSample(C.Structure):
    """struct somi_aug_sample."""
    _fields_ = [('canvas', AugCanvas * 2), ('mix', C.c_int32), ('hsv', C.c_int32), ('flipud', C.c_int32), ('fliplr', C.c_int32),
                ('mix_r', C.c_double), ('lut', (C.c_uint8 * 256) * 3)]


I, F, P, S, Z, U64 = C.c_int, C.c_float, C.c_void_p, c_stream, C.c_size_t, C.c_uint64

# name -> (restype, argtypes); every symbol include/somi_hip.h declares
SIGNATURES = {
    'somi_abi_version': (I, []),
    'somi_last_error': (C.c_char_p, []),
    'somi_sizeof_desc': (Z, [I]),
    'somi_conv2d_nhwc_f32': (I, [C.POINTER(ConvDesc), S]),
    'somi_conv2d_workspace_bytes': (Z, []),
    'somi_conv2d_stat_rows': (I, [C.POINTER(ConvDesc)]),
    'somi_conv2d_dgrad_nhwc_f32': (I, [C.POINTER(ConvDesc), P, I, I, P, P, I, I, P, I, I, S]),
    'somi_conv2d_wgrad_workspace_bytes': (Z, [C.POINTER(ConvDesc)]),
    'somi_conv2d_wgrad_nhwc_f32': (I, [C.POINTER(ConvDesc), P, I, I, P, I, I, P, P, P, Z, S]),
    'somi_conv2d_kernel_name': (C.c_char_p, [C.POINTER(ConvDesc)]),
    'somi_conv2d_wgrad_kernel_name': (C.c_char_p, [C.POINTER(ConvDesc)]),
    'somi_dcnv3_forward_f32': (I, [P, P, P, P] + [I] * 13 + [F, I, S]),
    'somi_dcnv3_backward_workspace_bytes': (Z, [I] * 13 + [F]),
    'somi_dcnv3_backward_f32': (I, [P, P, P, P, P, P, P] + [I] * 13 + [F, I, P, Z, S]),
    'somi_dcnv3_forward_strided_f32': (I, [P, P, P, C.c_long, C.c_long, P] + [I] * 13 + [F, I, S]),
    'somi_dcnv3_backward_strided_f32': (I, [P, P, P, C.c_long, C.c_long, P, P, P, P] + [I] * 13 + [F, I, P, Z, S]),
    'somi_dcnv3_forward_f16': (I, [P, P, P, P] + [I] * 13 + [F, I, S]),
    'somi_dcnv3_backward_f16': (I, [P, P, P, P, P, P, P] + [I] * 13 + [F, I, P, Z, S]),
    'somi_dcnv3_forward_f64': (I, [P, P, P, P] + [I] * 13 + [F, I, S]),
    'somi_dcnv3_backward_f64': (I, [P, P, P, P, P, P, P] + [I] * 13 + [F, I, P, Z, S]),
    'somi_layernorm_act_nhwc_f32': (I, [P, P, P, F, I, P, C.c_long, I, S]),
    'somi_dwconv3x3_ln_nhwc_f32': (I, [P, P, P, P, P, F, I, P, P, I, I, I, I, S]),
    'somi_group_softmax_f32': (I, [P, P, C.c_long, I, S]),
    'somi_group_softmax_strided_f32': (I, [P, C.c_long, P, C.c_long, C.c_long, I, I, S]),
    'somi_group_softmax_bwd_strided_f32': (I, [P, C.c_long, P, P, C.c_long, C.c_long, I, I, S]),
    'somi_layernorm_act_bwd_workspace_floats': (Z, [C.c_long, I]),
    'somi_layernorm_gelu_bwd_nhwc_f32': (I, [P, P, P, F, P, P, P, P, P, C.c_long, I, S]),
    'somi_group_softmax_bwd_f32': (I, [P, P, P, C.c_long, I, S]),
    'somi_dcnv3_cfs_blend_bwd_f32': (I, [P, P, P, I, P, P, P, P, I, C.c_long, I, I, S]),
    'somi_dcnv3_cfs_blend_f32': (I, [P, P, P, I, P, C.c_long, I, I, S]),
    'somi_image_u8_to_nhwc4': (I, [P, P, I, I, I, I, S]),
    'somi_image_f32_to_nhwc4': (I, [P, P, I, I, I, I, F, S]),
    'somi_dwconv3x3_nhwc_f32': (I, [P, P, P, P, P, P, P, I, I, I, I, I, S]),
    'somi_sppf_pool_nhwc_f32': (I, [P, I, I, I, I, I, I, S]),
    'somi_bifpn_nhwc_f32': (I, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), P, F, I, P, I, I, I, I, S]),
    'somi_pool_nchunk': (I, [I]),
    'somi_global_pool_nhwc_f32': (I, [P, I, I, I, I, I, P, P, P, S]),
    'somi_global_pool_act_nhwc_f32': (I, [P, I, I, I, I, I, I, P, P, P, P, S]),
    'somi_affine_silu_pool_rows': (I, [I, I, I]),
    'somi_affine_silu_pool_nhwc_f32': (I, [P, I, I, P, P, P, I, I, I, I, I, P, P, P, S]),
    'somi_attn_mlp_f32': (I, [I, P, P, P, P, P, P, P, I, I, I, S]),
    'somi_chan_stats_nhwc_f32': (I, [P, I, I, P, P, I, I, I, S]),
    'somi_spatial_attn_f32': (I, [P, P, P, P, I, I, I, I, S]),
    'somi_cbam_apply_nhwc_f32': (I, [P, I, I, P, P, P, P, P, I, I, I, I, I, I, I, S]),
    'somi_scale_channels_nhwc_f32': (I, [P, P, P, P, I, I, I, S]),
    'somi_odconv_weights_f32': (I, [P] * 18 + [I] * 7 + [S]),
    'somi_detect_decode_f32': (I, [P, I, P, I, C.POINTER(C.c_float), F, P, P, I, I, I, I, I, I, I, S]),
    'somi_red_nchunk': (I, [C.c_long]),
    'somi_bn_stats_nhwc_f32': (I, [P, I, I, C.c_long, I, F, F, P, P, P, P, P, P, P, P, P, S]),
    'somi_bn_stats_act_nhwc_f32': (I, [P, I, I, I, C.c_long, I, F, F, P, P, P, P, P, P, P, P, P, S]),
    'somi_bn_stats_partials_f32': (I, [P, P, I, C.c_long, I, F, F, P, P, P, P, P, P, P, P, P, S]),
    'somi_bn_local_sums_f64': (I, [P, I, I, C.c_long, I, P, P, P, I, P, P, S]),
    'somi_bn_stats_from_sums_f64': (I, [P, I, I, F, F, P, P, P, P, P, P, P, P, S]),
    'somi_bn_act_backward_sums_f64': (I, [P, I, I, P, I, I, P, P, P, I, I, C.c_long, I, P, P, S]),
    'somi_bn_act_backward_apply_sync_f32': (I, [P, I, I, P, I, I, P, P, P, P, I, I, P, P, I, P, I, I, P, P, C.c_long, I, P, S]),
    'somi_chan_affine_act_nhwc_f32': (I, [P, I, I, P, P, I, I, P, I, I, C.c_long, I, P, I, I, S]),
    'somi_bn_act_backward_nhwc_f32': (I, [P, I, I, P, I, I, P, P, P, P, I, I, I, P, I, I, P, P, C.c_long, I, P, S]),
    'somi_bn_pooled_rows': (I, [I, I]),
    'somi_bn_act_backward_pooled_nhwc_f32': (I, [P, I, I, P, I, I, P, P, P, P, I, I, P, P, P, P, I, I, P, P, I, I, I, P, S]),
    'somi_add_nhwc_f32': (I, [P, I, I, P, I, I, P, I, I, C.c_long, I, S]),
    'somi_chan_sum_nhwc_f32': (I, [P, I, I, C.c_long, I, P, P, S]),
    'somi_img_nchunk': (I, [I]),
    'somi_cbam_bwd_pixel_argmax_f32': (I, [P, I, I, P, I, I, P, P, P, P, P, P, I, I, I, S]),
    'somi_cbam_bn_bwd_workspace_floats': (C.c_size_t, [I, I, I]),
    'somi_cbam_bn_bwd_reduce_f32': (I, [P, I, I, P, I, I, P, P, P, P, P, P, P, P, P, P, I, I, I, S]),
    'somi_cbam_bn_bwd_apply_f32': (I, [P, I, I, P, I, I, P, P, P, P, P, P, P, P, P, P, P, P, I, I, P, P, P, I, I, I, S]),
    'somi_spatial_attn_bwd_f32': (I, [P, P, P, P, P, P, P, I, I, I, I, I, S]),
    'somi_cbam_bwd_chan_f32': (I, [P, I, I, P, I, I, P, P, P, P, P, P, I, I, I, S]),
    'somi_attn_mlp_bwd_workspace_floats': (Z, [I, I, I]),
    'somi_attn_mlp_bwd_f32': (I, [I, P, P, P, P, P, P, P, P, P, P, P, P, P, P, I, I, I, S]),
    'somi_pool_bwd_add_nhwc_f32': (I, [P, I, I, P, P, P, I, I, I, S]),
    'somi_detect_raw_bwd_f32': (I, [P, P, I, P, I, I, I, I, I, I, S]),
    'somi_resample_slice_nhwc_f32': (I, [P, I, I, P, I, I, I, I, I, I, I, I, I, S]),
    'somi_space_to_depth_nhwc_f32': (I, [P, I, I, P, I, I, I, I, I, I, I, S]),
    'somi_detect_plain_decode_f32': (I, [P, I, C.POINTER(C.c_float), F, P, P, I, I, I, I, I, I, I, S]),
    'somi_detect_plain_raw_bwd_f32': (I, [P, P, I, I, I, I, I, I, S]),
    'somi_tta_resample_nhwc4_f32': (I, [P, P, I, I, I, I, I, I, I, I, F, I, S]),
    'somi_tta_descale_f32': (I, [P, C.c_long, I, F, I, F, S]),
    'somi_sppf_pool_bwd_nhwc_f32': (I, [P, P, P, I, I, I, I, I, I, S]),
    'somi_sppf_pool_codes_nhwc_f32': (I, [P, P, I, I, I, I, I, I, S]),
    'somi_bifpn_bwd_nhwc_f32': (I, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int), P, F, I, P, P, P, I, I, I, I, S]),
    'somi_dwconv3x3_bwd_workspace_floats': (Z, [I, I, I]),
    'somi_dwconv3x3_bwd_nhwc_f32': (I, [P, P, P, P, P, P, P, P, I, I, I, I, S]),
    'somi_scale_channels_bwd_nhwc_f32': (I, [P, P, P, P, P, P, I, I, I, S]),
    'somi_linear_f32': (I, [P, I, P, P, I, P, I, I, I, I, I, S]),
    'somi_linear_bwd_f32': (I, [P, I, P, P, P, I, I, I, P, P, P, I, I, P, I, I, I, S]),
    'somi_odconv_synth_f32': (I, [P, P, P, P, P, I, I, I, I, I, I, S]),
    'somi_odconv_synth_bwd_workspace_floats': (Z, [I, I, I, I, I]),
    'somi_odconv_synth_bwd_f32': (I, [P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, S]),
    'somi_adam_ema_step_f32': (I, [P, P, P, P, P, C.c_long, F, F, F, F, F, I, F, S]),
    'somi_sgd_ema_step_f32': (I, [P, P, P, P, C.c_long, F, F, F, I, F, S]),
    'somi_pack_dgrad_weights_f32': (I, [P, P, I, I, I, S]),
    'somi_gconv2d_stat_rows': (I, [I, I, I, I]),
    'somi_gconv2d_nhwc_f32': (I, [P, I, I, I, I, I, I, P, I, P, I, I, I, P, I, I, I, I, I, P, I, I, P, P, P, S]),
    'somi_gconv2d_dgrad_nhwc_f32': (I, [P, I, I, I, I, I, I, P, I, I, I, I, P, I, I, I, I, I, I, P, I, I, P, I, I, S]),
    'somi_gconv2d_wgrad_workspace_floats': (Z, [I, I, I, I, I, I]),
    'somi_gconv2d_wgrad_nhwc_f32': (I, [P, I, I, I, I, I, I, P, I, I, I, I, I, I, I, I, P, I, P, Z, S]),
    'somi_dwlk_strip_length': (I, []),
    'somi_dwlk_strips_per_workgroup': (I, [I, I, I, I, I]),
    'somi_dwlk_stat_rows': (I, [I, I, I, I]),
    'somi_dwlk_nhwc_f32': (I, [Slice, P, I, P, I, I, P, P, Slice, Slice, I, I, I, I, P, P, P, S]),
    'somi_dwlk_dgrad_nhwc_f32': (I, [Slice, P, I, I, Slice, Slice, Slice, I, I, I, I, S]),
    'somi_dwlk_wgrad_workspace_floats': (Z, [I, I, I, I, I]),
    'somi_dwlk_wgrad_nhwc_f32': (I, [Slice, Slice, I, I, I, I, I, P, P, I, P, Z, S]),
    'somi_psa_attention_f32': (I, [P, I, I, I, I, I, P, I, I, P, P, S]),
    'somi_psa_attention_backward_f32': (I, [P, I, I, P, I, I, P, I, I, P, I, I, I, P, I, I, P, P, S]),
    'somi_swin_attention_lse_floats': (Z, [I, I, I, I]),
    'somi_swin_attention_f32': (I, [P, P, P, I, I, I, I, I, I, P, P, S]),
    'somi_swin_attention_bwd_workspace_floats': (Z, [I, I, I, I]),
    'somi_swin_attention_backward_f32': (I, [P, P, P, P, P, I, I, I, I, I, I, P, P, P, S]),
    'somi_layernorm_bwd_workspace_floats': (Z, [C.c_long, I]),
    'somi_layernorm_bwd_nhwc_f32': (I, [P, P, F, P, P, P, P, P, P, C.c_long, I, S]),
    'somi_gelu_bwd_f32': (I, [P, P, P, C.c_long, S]),
    'somi_axpby_f32': (I, [P, P, C.c_long, F, F, S]),
    'somi_nms_workspace_bytes': (Z, [I, I, I, I]),
    'somi_nms_f32': (I, [P, I, I, I, F, F, I, I, P, I, P, P, P, Z, S]),
    'somi_nms_ex_workspace_bytes': (Z, [I, I, I, I, I, I]),
    'somi_nms_ex_f32': (I, [P, I, I, I, F, F, I, I, P, I, I, I, F, F, P, P, P, Z, S]),
    'somi_nms_boxes_workspace_bytes': (Z, [I]),
    'somi_nms_boxes_f32': (I, [P, P, I, I, F, F, F, P, P, P, Z, S]),
    'somi_loss_workspace_bytes': (Z, [C.POINTER(LossDesc)]),
    'somi_yolo_loss_f32': (I, [C.POINTER(LossDesc), P, P, Z, S]),
    'somi_loss5_workspace_bytes': (Z, [C.POINTER(LossDesc), C.POINTER(LossLevel)]),
    'somi_yolo_loss5_f32': (I, [C.POINTER(LossDesc), C.POINTER(LossLevel), P, P, Z, S]),
    'somi_loss_rule_workspace_bytes': (Z, [C.POINTER(LossDesc), C.POINTER(LossLevel), C.POINTER(LossBoxRule)]),
    'somi_yolo_loss_rule_f32': (I, [C.POINTER(LossDesc), C.POINTER(LossLevel), C.POINTER(LossBoxRule), P, P, Z, S]),
    'somi_maxpool2_nhwc_f32': (I, [P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, S]),
    'somi_maxpool2_bwd_nhwc_f32': (I, [P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, S]),
    'somi_maxpool3s2_nhwc_f32': (I, [C.POINTER(Slice), C.POINTER(Slice), P, I, I, I, I, S]),
    'somi_maxpool3s2_bwd_nhwc_f32': (I, [C.POINTER(Slice), P, C.POINTER(Slice), I, I, I, I, S]),
    'somi_asff_desc_bytes': (Z, []),
    'somi_asff_fuse_bwd_workspace_floats': (Z, [I, I, I]),
    'somi_asff_fuse_nhwc_f32': (I, [C.POINTER(AsffDesc), S]),
    'somi_asff_fuse_bwd_nhwc_f32': (I, [C.POINTER(AsffDesc), S]),
    'somi_coordatt_desc_bytes': (Z, []),
    'somi_coordatt_workspace_floats': (Z, [I, I, I, I]),
    'somi_coordatt_means_nhwc_f32': (I, [C.POINTER(CoordAttDesc), S]),
    'somi_coordatt_apply_nhwc_f32': (I, [C.POINTER(CoordAttDesc), S]),
    'somi_coordatt_bwd_gates_nhwc_f32': (I, [C.POINTER(CoordAttDesc), S]),
    'somi_coordatt_bwd_input_nhwc_f32': (I, [C.POINTER(CoordAttDesc), S]),
    'somi_ema_desc_bytes': (Z, []),
    'somi_ema_workspace_floats': (Z, [I, I, I, I]),
    'somi_ema_partials': (I, [I, I, I, I]),
    'somi_ema_stats_nhwc_f32': (I, [C.POINTER(EmaDesc), S]),
    'somi_ema_gate_nhwc_f32': (I, [C.POINTER(EmaDesc), S]),
    'somi_ema_bwd_gate_nhwc_f32': (I, [C.POINTER(EmaDesc), S]),
    'somi_ema_bwd_norm_nhwc_f32': (I, [C.POINTER(EmaDesc), S]),
    'somi_acmix_desc_bytes': (Z, []),
    'somi_acmix_workspace_floats': (Z, [I, I, I, I]),
    'somi_acmix_plan': (I, [I, I, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'somi_acmix_attn_nhwc_f32': (I, [C.POINTER(AcmixDesc), S]),
    'somi_acmix_attn_bwd_q_nhwc_f32': (I, [C.POINTER(AcmixDesc), S]),
    'somi_acmix_attn_bwd_kv_nhwc_f32': (I, [C.POINTER(AcmixDesc), S]),
    'somi_acmix_conv_nhwc_f32': (I, [C.POINTER(AcmixDesc), S]),
    'somi_acmix_conv_bwd_data_nhwc_f32': (I, [C.POINTER(AcmixDesc), S]),
    'somi_acmix_conv_bwd_weight_nhwc_f32': (I, [C.POINTER(AcmixDesc), S]),
    'somi_acmix_fold_weff_f32': (I, [P, P, P, I, S]),
    'somi_acmix_split_dweff_f32': (I, [P, P, P, P, P, I, S]),
    'somi_cpca_strip_desc_bytes': (Z, []),
    'somi_cpca_wgrad_desc_bytes': (Z, []),
    'somi_cpca_fanout_nhwc_f32': (I, [C.POINTER(CpcaStripDesc), S]),
    'somi_cpca_fanin_nhwc_f32': (I, [C.POINTER(CpcaStripDesc), S]),
    'somi_cpca_wgrad_workspace_floats': (Z, [I, I, I, I]),
    'somi_cpca_tiles_per_workgroup': (I, [I, I, I, I, I, I]),
    'somi_cpca_wgrad_nhwc_f32': (I, [C.POINTER(CpcaWgradDesc), S]),
    'somi_cpca_gate_nhwc_f32': (I, [Slice, Slice, Slice, C.c_long, I, S]),
    'somi_cpca_gate_bwd_nhwc_f32': (I, [Slice, Slice, Slice, Slice, Slice, C.c_long, I, S]),
    'somi_cpca_sigmoid2_f32': (I, [P, P, I, I, S]),
    'somi_cpca_sigmoid2_bwd_f32': (I, [P, P, P, I, I, S]),
    'somi_cpca_argmax_pixel_nhwc_f32': (I, [Slice, P, P, I, I, I, S]),
    'somi_gate_combine_nhwc_f32': (I, [Slice, P, P, Slice, Slice, I, I, I, I, S]),
    'somi_gate_combine_bwd_pixel_f32': (I, [Slice, Slice, P, P, P, P, P, P, I, I, I, I, I, S]),
    'somi_gate_combine_bwd_workspace_floats': (Z, [I, I, I]),
    'somi_gate_combine_pixel_trips': (I, [I, I, I]),
    'somi_dwc_gate_workspace_floats': (Z, [I, I, I, I]),
    'somi_dwc_gate_trips': (I, [I, I, I]),
    'somi_dwc_gate_eval_f32': (I, [P, P, P, P, I, I, I, I, F, S]),
    'somi_dwc_gate_train_f32': (I, [P, P, P, P, P, P, F, F, P, P, Z, I, I, I, I, S]),
    'somi_dwc_gate_bwd_f32': (I, [P, P, P, P, P, P, P, P, P, Z, I, I, I, I, S]),
    'somi_gate_combine_bwd_chan_f32': (I, [Slice, Slice, P, P, P, P, Slice, P, P, Z, I, I, I, I, I, S]),
    'somi_simam_desc_bytes': (Z, []),
    'somi_simam_workspace_floats': (Z, [C.POINTER(SimamDesc)]),
    'somi_simam_stats_nhwc_f32': (I, [C.POINTER(SimamDesc), S]),
    'somi_simam_apply_nhwc_f32': (I, [C.POINTER(SimamDesc), S]),
    'somi_simam_bwd_sums_nhwc_f32': (I, [C.POINTER(SimamDesc), S]),
    'somi_simam_bwd_input_nhwc_f32': (I, [C.POINTER(SimamDesc), S]),
    'somi_zoomcat_desc_bytes': (Z, []),
    'somi_zoomcat_nhwc_f32': (I, [C.POINTER(ZoomcatDesc), S]),
    'somi_zoomcat_bwd_nhwc_f32': (I, [C.POINTER(ZoomcatDesc), S]),
    'somi_scalseq_desc_bytes': (Z, []),
    'somi_scalseq_workspace_floats': (Z, [I, I, I, I]),
    'somi_scalseq_stats_f32': (I, [C.POINTER(ScalseqDesc), S]),
    'somi_scalseq_fuse_nhwc_f32': (I, [C.POINTER(ScalseqDesc), S]),
    'somi_scalseq_route_bwd_nhwc_f32': (I, [C.POINTER(ScalseqDesc), S]),
    'somi_scalseq_apply_bwd_f32': (I, [C.POINTER(ScalseqDesc), S]),
    'somi_asfatt_desc_bytes': (Z, []),
    'somi_asfatt_workspace_floats': (Z, [I, I, I, I]),
    'somi_eca_gate_f32': (I, [P, P, I, P, I, I, S]),
    'somi_eca_gate_bwd_f32': (I, [P, P, I, P, P, P, P, I, I, S]),
    'somi_asf_mix_means_nhwc_f32': (I, [C.POINTER(AsfAttDesc), S]),
    'somi_asf_mix_bwd_sums_nhwc_f32': (I, [C.POINTER(AsfAttDesc), S]),
    'somi_asf_mix_bwd_input_nhwc_f32': (I, [C.POINTER(AsfAttDesc), S]),
    'somi_gs_tiles_per_workgroup': (I, [C.c_long, I]),
    'somi_gs_tail_nhwc_f32': (I, [Slice, P, P, P, P, I, I, Slice, Slice, I, I, I, I, S]),
    'somi_gs_shuffle_affine_act_nhwc_f32': (I, [Slice, Slice, P, P, I, Slice, Slice, C.c_long, I, S]),
    'somi_gs_unshuffle_nhwc_f32': (I, [Slice, Slice, Slice, C.c_long, I, S]),
    'somi_spp_pool_nhwc_f32':(I, [P, P, I, I, I, I, I, I, I, I, I, I, S]),
    'somi_spp_pool_bwd_nhwc_f32': (I, [P, P, I, I, I, I, I, I, I, I, I, I, S]),
    'somi_carafe_nhwc_f32': (I, [P, P, P, P] + [I] * 11 + [S]),
    'somi_carafe_bwd_nhwc_f32': (I, [P, P, P, P, P] + [I] * 13 + [S]),
    'somi_dysample_nhwc_f32': (I, [P, P, P, P] + [I] * 11 + [S]),
    'somi_dysample_bwd_nhwc_f32': (I, [P, P, P, P, P, P, P] + [I] * 15 + [S]),
    'somi_val_match_f32': (I, [P, P, P, P, P, I, I, I, I, P, S]),
    'somi_confusion_matrix_f32': (I, [P, P, P, P, I, I, I, I, F, F, P, S]),
    'somi_ap_per_class_workspace_bytes': (Z, [C.c_long, I, I]),
    'somi_ap_per_class_f64': (I, [P, P, P, P, C.c_long, C.c_long, I, I, P, P, P, P, P, P, P, Z, S]),
    'somi_repulsion_workspace_bytes': (Z, [I, I]),
    'somi_repulsion_loss_f32': (I, [P, P, P, I, I, F, F, F, F, P, P, Z, S]),
    'somi_wbf_workspace_bytes': (Z, [I]),
    'somi_augment_u8': (I, [P, I, I, I, I, P, S]),
    'somi_wbf_f32': (I, [P, P, P, P, I, I, C.POINTER(C.c_float), F, F, P, P, P, P, P, Z, S]),
    'somi_wbf_batch_workspace_bytes': (Z, [I, I, I]),
    'somi_wbf_batch_f32': (I, [C.POINTER(P), C.POINTER(P), I, I, I, C.POINTER(C.c_float), F, F, F, F, P, P, P, P, P, Z, S]),
    'somi_anchor_metric_workspace_bytes': (Z, [C.c_long]),
    'somi_anchor_metric_f32': (I, [P, C.c_long, P, I, F, P, P, P, Z, S]),
    'somi_anchor_evolve_f32': (I, [P, C.c_long, P, I, P, I, F, P, P, P, Z, S]),
    'somi_kmeans_workspace_bytes': (Z, [C.c_long, I, I]),
    'somi_kmeans_lloyd_step_f64': (I, [P, C.c_long, P, P, I, I, C.c_double, P, P, P, P, Z, S]),
}

_lib = None


def lib():
    """The loaded library (loads on first use; raises if it is not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                               f'(or `make -C yolo-somi_amd/csrc`). There is no CPU fallback.')
        # torch first: its wheel carries its own libamdhip64.so (SONAME libamdhip64.so.7) and asks for it by the name "libamdhip64.so".  Loaded
        # before torch, this library would pull /opt/rocm's copy under its SONAME, torch's request would not match that name and a SECOND HIP
        # runtime would come up in the process - whose launches then fail with "no ROCm-capable device is detected".  With torch's copy mapped
        # first, the SONAME this library asks for resolves to it and there is one runtime.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        lax = bool(os.environ.get('SOMI_HIP_LIB')) and os.environ.get('SOMI_HIP_LIB_LAX') == '1'   # kernel A/B runs against an older build
        for name, (res, args) in SIGNATURES.items():
            if lax and not hasattr(L, name):
                continue
            fn = getattr(L, name)            # AttributeError here = header/library mismatch: fail loudly
            fn.restype, fn.argtypes = res, args
        if L.somi_abi_version() != ABI_VERSION and not lax:
            raise RuntimeError('libsomi_hip.so ABI version mismatch')
        if not lax and (L.somi_sizeof_desc(0) != C.sizeof(ConvDesc) or L.somi_sizeof_desc(1) != C.sizeof(LossDesc)
                        or L.somi_sizeof_desc(2) != C.sizeof(LossBoxRule) or L.somi_asff_desc_bytes() != C.sizeof(AsffDesc)
                        or L.somi_coordatt_desc_bytes() != C.sizeof(CoordAttDesc)
                        or L.somi_ema_desc_bytes() != C.sizeof(EmaDesc)
                        or L.somi_acmix_desc_bytes() != C.sizeof(AcmixDesc)
                        or L.somi_cpca_strip_desc_bytes() != C.sizeof(CpcaStripDesc)
                        or L.somi_cpca_wgrad_desc_bytes() != C.sizeof(CpcaWgradDesc)
                        or L.somi_simam_desc_bytes() != C.sizeof(SimamDesc)
                        or L.somi_zoomcat_desc_bytes() != C.sizeof(ZoomcatDesc)
                        or L.somi_scalseq_desc_bytes() != C.sizeof(ScalseqDesc)
                        or L.somi_asfatt_desc_bytes() != C.sizeof(AsfAttDesc)):
            raise RuntimeError('libsomi_hip.so descriptor layout differs from this binding')
        _lib = L
    return _lib


def check(rc, what=''):
    if rc != 0:
        msg = lib().somi_last_error().decode(errors='replace')
        raise RuntimeError(f'{what or "somi"} failed (code {rc}): {msg}')
