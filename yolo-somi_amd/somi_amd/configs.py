"""Configuration data of the SOMI path and deterministic synthetic weights (product side).

`somi_cfg` is the layer table of models/modules/YOLO-SOMI.yaml as a dict (with the documented C2fEACBAM -> C2fCBAM
substitution, SURVEY.md "five facts" #2), `SOMI_ANCHORS` the 16 anchor pairs of its line 9 comment, `HYP_VISDRONE` the
loss-relevant keys of data/hyps/hyp.VisDrone.yaml.  `fill_state` gives every parameter a value derived from its
state_dict name (bench.py's synthetic weights: no checkpoint can be downloaded here); `synthetic_batch` is the
VisDrone-shaped batch of SURVEY.md section 8d.
"""
import math
import zlib

import numpy as np
import torch


def fill_state(module, seed=0):
    """In-place deterministic fill of module.state_dict(); returns the module."""
    with torch.no_grad():
        for name, t in module.state_dict().items():
            if not t.dtype.is_floating_point:
                continue                                        # num_batches_tracked etc.
            g = torch.Generator().manual_seed((zlib.crc32(name.encode()) + 7919 * seed) & 0x7FFFFFFF)
            leaf = name.rsplit('.', 1)[-1]
            if leaf == 'running_var':
                v = torch.rand(t.shape, generator=g) + 0.5       # U(0.5, 1.5)
            elif leaf == 'running_mean':
                v = torch.randn(t.shape, generator=g) * 0.1
            elif leaf == 'anchors':
                continue                                        # geometry, not a weight
            elif t.dim() == 1 and leaf == 'weight':              # BN / LN scale (BiFPN weight too)
                v = torch.rand(t.shape, generator=g) + 0.5
            elif t.dim() <= 1 or leaf == 'bias':
                v = torch.randn(t.shape, generator=g) * 0.1
            else:                                               # conv / linear / ODConv kernels
                fan_in = t[0].numel() if t.dim() < 5 else t[0, 0].numel()
                v = torch.randn(t.shape, generator=g) * (1.0 / math.sqrt(max(fan_in, 1)))
            t.copy_(v.to(t.dtype))
    return module


def synthetic_batch(batch, size, nc=10, seed=0):
    """uint8 images (B,3,S,S) and targets (nt,6) = [img, cls, x, y, w, h] as SURVEY.md section 8d specifies."""
    rng = np.random.RandomState(seed)
    imgs = torch.from_numpy(rng.randint(0, 256, (batch, 3, size, size), dtype=np.uint8))
    rows = []
    for b in range(batch):
        n = int(np.clip(rng.poisson(54), 1, 300))
        cls = rng.randint(0, nc, n).astype(np.float32)
        xy = rng.uniform(0.02, 0.98, (n, 2)).astype(np.float32)
        wh = np.clip(np.exp(rng.normal(math.log(0.03), 0.7, (n, 2))), 0.004, 0.5).astype(np.float32)
        rows.append(np.concatenate([np.full((n, 1), b, np.float32), cls[:, None], xy, wh], 1))
    return imgs, torch.from_numpy(np.concatenate(rows, 0))


SOMI_ANCHORS = [[4, 6, 12, 8, 7, 14, 20, 12], [13, 22, 31, 18, 21, 33, 46, 23],
                [37, 37, 31, 56, 65, 34, 55, 57], [95, 52, 60, 90, 147, 76, 103, 134]]
"""The 16 anchor pairs listed in models/modules/YOLO-SOMI.yaml:9 (comment), 4 per level P2..P5."""

HYP_VISDRONE = dict(lr0=0.0032, lrf=0.12, momentum=0.843, weight_decay=0.00036, warmup_epochs=2.0,
                    warmup_momentum=0.5, warmup_bias_lr=0.05, box=0.07, cls=0.18, cls_pw=0.631, obj=0.15,
                    obj_pw=0.911, iou_t=0.2, anchor_t=3, fl_gamma=0.0, alpha=0.01, beta=0.1, Rp_nms=0.1,
                    deta=0.5, slide_ratio=0, nwdloss=0, shapeloss=0, label_smoothing=0.0)
"""Loss-relevant keys of data/hyps/hyp.VisDrone.yaml (values are configuration data)."""


UPSAMPLE_ROWS = {'nearest': None, 'carafe': ['CARAFE', [3, 5]], 'dysample': ['DySample', []]}
"""upsample= of somi_cfg / yolov5_cfg / yolov10_cfg -> what stands in the tables' nn.Upsample rows: the reference's two learned 2x drop-ins
(models/common.py:4450 CARAFE with its docstring's [3, 5] = k_enc, k_up; :4246 DySample with its defaults) or the rows as they are."""


def _swap_upsample(rows, upsample):
    """Rewrites every nn.Upsample row of a layer table in place (same `from`, same output size and channels: nothing else moves)."""
    if upsample not in UPSAMPLE_ROWS:
        raise ValueError(f'upsample={upsample!r} (one of {sorted(UPSAMPLE_ROWS)})')
    swap = UPSAMPLE_ROWS[upsample]
    if swap is None:
        return rows
    import copy
    return [[r[0], r[1], *copy.deepcopy(swap)] if r[2] == 'nn.Upsample' else r for r in rows]


def somi_cfg(width=1.0, depth=1.0, nc=10, anchors=4, dcn=False, dcn_group=8, upsample='nearest', seam='seam', seam_depth=1):
    """The layer table of models/modules/YOLO-SOMI.yaml as a dict (C2fEACBAM -> C2fCBAM).

    dcn=True: "yolov5l-SOMI (DCNv3 blocks)" of BASELINE configs[1].  The reference vendors DCNv3 but wires it into no yaml (SURVEY
    fact 3), so the sites are the build's choice: one DCNv3_YOLO block (DCNv3 -> BN -> SiLU, 3x3, `dcn_group` groups) behind each of
    the two high-resolution lateral convs of the neck - P2 (160x160 at 640) and P3 (80x80), 256 channels: the representative
    shapes of SURVEY section 8a row F10.  Later layers shift by one / two; their `from` indices are rewritten accordingly.
    upsample='carafe' | 'dysample': the neck's three nn.Upsample rows become the learned upsampler (UPSAMPLE_ROWS).
    seam='multi': the neck's three SEAM rows become MultiSEAM (models/common.py:8527-8555, registered beside SEAM at models/yolo.py:1475) with
    `seam_depth` stages per branch; seam='seam' with seam_depth > 1: SEAM with that many stages.  The defaults give the shipped table."""
    if seam not in ('seam', 'multi'):
        raise ValueError(f"seam={seam!r} ('seam' or 'multi')")
    if not isinstance(seam_depth, int) or seam_depth < 1:
        raise ValueError(f'seam_depth={seam_depth!r} (an int >= 1)')
    bb = [[-1, 1, 'Conv', [64, 3, 2]], [-1, 1, 'ODConv_3rd', [128, 3, 2, 4]], [-1, 3, 'C2fCBAM', [128, True]],
          [-1, 1, 'Conv', [256, 3, 2]], [-1, 6, 'C2fCBAM', [256, True]], [-1, 1, 'Conv', [512, 3, 2]],
          [-1, 6, 'C2fCBAM', [512, True]], [-1, 1, 'Conv', [1024, 3, 2]], [-1, 3, 'C2fCBAM', [1024, True]],
          [-1, 1, 'SPPF', [1024, 5]]]
    up = [-1, 1, 'nn.Upsample', [None, 2, 'nearest']]
    hd = [[2, 1, 'Conv', [256]], [4, 1, 'Conv', [256]], [6, 1, 'Conv', [256]], [9, 1, 'Conv', [256]],
          up, [[-1, 12], 1, 'BiFPN', []], [-1, 1, 'SEAM', [256, 1, 16]], [-1, 3, 'C2fCBAM', [256]],
          up, [[-1, 11], 1, 'BiFPN', []], [-1, 1, 'SEAM', [256, 1, 16]], [-1, 3, 'C2fCBAM', [256]],
          up, [[-1, 10], 1, 'BiFPN', []], [-1, 1, 'SEAM', [256, 1, 16]], [-1, 3, 'C2fCBAM', [256]],
          [-1, 1, 'ODConv_3rd', [256, 3, 2, 4]], [[-1, 11, 21], 1, 'BiFPN', []], [-1, 3, 'C2fCBAM', [256]],
          [-1, 1, 'ODConv_3rd', [256, 3, 2, 4]], [[-1, 12, 17], 1, 'BiFPN', []], [-1, 3, 'C2fCBAM', [512]],
          [-1, 1, 'ODConv_3rd', [256, 3, 2, 4]], [[-1, 13], 1, 'BiFPN', []], [-1, 3, 'C2fCBAM', [1024]],
          [[25, 28, 31, 34], 1, 'DecoupledDetect', ['nc', 'anchors']]]
    import copy
    bb, hd = copy.deepcopy(bb), copy.deepcopy(hd)
    if seam == 'multi' or seam_depth > 1:
        for l in hd:
            if l[2] == 'SEAM':
                l[2:] = ['MultiSEAM', [256, seam_depth]] if seam == 'multi' else ['SEAM', [256, seam_depth, 16]]
    if dcn:
        layers = bb + hd
        for after in (11, 10):                                   # insert behind layer 11 first, so that index 10 stays valid
            for l in layers:                                     # absolute references to later layers move up by one
                l[0] = [j + 1 if j > after else j for j in l[0]] if isinstance(l[0], list) else (l[0] + 1 if l[0] > after else l[0])
            layers.insert(after + 1, [after, 1, 'DCNv3_YOLO', [256, 3, 1, dcn_group]])
        # the lateral convs' other consumers (the BiFPN inputs) now read the DCNv3 output: references to 10 / 11 move to 11 / 13
        for l in layers:
            if l[2] != 'DCNv3_YOLO':
                l[0] = [{10: 11, 12: 13}.get(j, j) for j in l[0]] if isinstance(l[0], list) else {10: 11, 12: 13}.get(l[0], l[0])
        bb, hd = layers[:len(bb)], layers[len(bb):]
    return dict(nc=nc, depth_multiple=depth, width_multiple=width, anchors=copy.deepcopy(anchors), backbone=bb, head=_swap_upsample(hd, upsample))


COCO_ANCHORS = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
"""The stock YOLOv5 P3-P5 anchors (upstream yolov5s.yaml; the reference ships no yolov5s.yaml, SURVEY section 2 #21)."""


HEADS = ('Detect', 'ASFF_Detect')


def yolov5_cfg(width=0.50, depth=0.33, nc=80, anchors=None, version='6.0', upsample='nearest', head='Detect'):
    """Stock YOLOv5 layer tables authored here (BASELINE configs[0]; the reference ships none): version '6.0' = Conv 6x6 stem + SPPF
    (upstream yolov5s.yaml of the release this fork is based on); '5.0' = Focus stem + SPP(5,9,13), which exercises the remaining
    stock modules.  Defaults are yolov5s (depth 0.33, width 0.50, 80 classes -> 7,235,389 parameters for '6.0').
    upsample='carafe' | 'dysample': the head's two nn.Upsample rows become the learned upsampler (UPSAMPLE_ROWS).
    head='ASFF_Detect': the last row names the reference's ASFF head (models/yolo.py:172-184) instead of Detect; it is built for width 0.50 only
    (levels of 128 / 256 / 512 channels)."""
    import copy
    if head not in HEADS:
        raise ValueError(f'head must be one of {HEADS}, got {head!r}')
    if version == '6.0':
        bb = [[-1, 1, 'Conv', [64, 6, 2, 2]], [-1, 1, 'Conv', [128, 3, 2]], [-1, 3, 'C3', [128]], [-1, 1, 'Conv', [256, 3, 2]],
              [-1, 6, 'C3', [256]], [-1, 1, 'Conv', [512, 3, 2]], [-1, 9, 'C3', [512]], [-1, 1, 'Conv', [1024, 3, 2]],
              [-1, 3, 'C3', [1024]], [-1, 1, 'SPPF', [1024, 5]]]
    else:
        bb = [[-1, 1, 'Focus', [64, 3]], [-1, 1, 'Conv', [128, 3, 2]], [-1, 3, 'C3', [128]], [-1, 1, 'Conv', [256, 3, 2]],
              [-1, 9, 'C3', [256]], [-1, 1, 'Conv', [512, 3, 2]], [-1, 9, 'C3', [512]], [-1, 1, 'Conv', [1024, 3, 2]],
              [-1, 1, 'SPP', [1024, [5, 9, 13]]], [-1, 3, 'C3', [1024, False]]]
    up = [-1, 1, 'nn.Upsample', [None, 2, 'nearest']]
    hd = [[-1, 1, 'Conv', [512, 1, 1]], up, [[-1, 6], 1, 'Concat', [1]], [-1, 3, 'C3', [512, False]],
          [-1, 1, 'Conv', [256, 1, 1]], up, [[-1, 4], 1, 'Concat', [1]], [-1, 3, 'C3', [256, False]],
          [-1, 1, 'Conv', [256, 3, 2]], [[-1, 14], 1, 'Concat', [1]], [-1, 3, 'C3', [512, False]],
          [-1, 1, 'Conv', [512, 3, 2]], [[-1, 10], 1, 'Concat', [1]], [-1, 3, 'C3', [1024, False]],
          [[17, 20, 23], 1, head, ['nc', 'anchors']]]
    return dict(nc=nc, depth_multiple=depth, width_multiple=width, anchors=copy.deepcopy(anchors or COCO_ANCHORS),
                backbone=copy.deepcopy(bb), head=_swap_upsample(copy.deepcopy(hd), upsample))


def yolov5_asf_cfg(depth=0.33, nc=80, anchors=None):
    """The v6.0 yolov5 backbone at width 1.0 with the ASF-YOLO head (attentional scale sequence fusion; models/common.py:4312-4424).  The
    reference registers Zoom_cat, ScalSeq and attention_model in its parser (models/yolo.py:1577-1582) but ships no yaml that names them.
    Width 1.0 is fixed: ScalSeq hard-codes 512 and 1024 input channels and the parser scales none of the three rows' arguments.  Every
    Zoom_cat takes three inputs of its named width at strides 2 : 1 : 1/2 (rows 12 and 16), ScalSeq reads 256, 512 and 1024 channels at
    strides 8, 16 and 32 (row 24), attention_model joins the P3 head row and ScalSeq's output (row 25), which Detect reads as its P3 level."""
    cfg = yolov5_cfg(1.0, depth, nc, anchors)
    cfg['head'] = [[-1, 1, 'Conv', [512, 1, 1]], [4, 1, 'Conv', [512, 1, 1]], [[-1, 6, -2], 1, 'Zoom_cat', [512]],
                   [-1, 3, 'C3', [512, False]], [-1, 1, 'Conv', [256, 1, 1]], [2, 1, 'Conv', [256, 1, 1]],
                   [[-1, 4, -2], 1, 'Zoom_cat', [256]], [-1, 3, 'C3', [256, False]], [-1, 1, 'Conv', [256, 3, 2]],
                   [[-1, 14], 1, 'Concat', [1]], [-1, 3, 'C3', [512, False]], [-1, 1, 'Conv', [512, 3, 2]],
                   [[-1, 10], 1, 'Concat', [1]], [-1, 3, 'C3', [1024, False]], [[4, 6, 8], 1, 'ScalSeq', [256]],
                   [[17, -1], 1, 'attention_model', [256]], [[25, 20, 23], 1, 'Detect', ['nc', 'anchors']]]
    return cfg


def yolov5_slimneck_cfg(width=0.50, depth=0.33, nc=80, anchors=None):
    """yolov5s 6.0 with the slim-neck head (GSConv, models/common.py:9586-9610; VoVGSCSPCBAM, :2697-2711).  The reference registers both in its
    parser (models/yolo.py:1473-1474, VoVGSCSPCBAM among the modules repeated inside, :1489) but ships no yaml that names them.  The head's
    four Conv rows become GSConv with the same arguments and its four C3 rows [c, False] VoVGSCSPCBAM with the same arguments and n; the
    backbone and Detect are yolov5_cfg's."""
    cfg = yolov5_cfg(width, depth, nc, anchors)
    for row in cfg['head']:
        row[2] = {'Conv': 'GSConv', 'C3': 'VoVGSCSPCBAM'}.get(row[2], row[2])
    return cfg


CONVNEXT_WHERE = {'cneb': 'CNeB', 'cspcm': 'CSPCM'}


def yolov5_convnext_cfg(width=0.50, depth=0.33, nc=80, anchors=None, where='cneb'):
    """yolov5s 6.0 whose four backbone C3 rows are the large-kernel depthwise blocks: where='cneb' the ConvNeXt C3 (CNeB, models/common.py:6780-6791,
    a 7x7 depthwise conv per block), where='cspcm' the ConvMixer C3 (CSPCM, :7169-7180, 9x9).  The reference registers both in its parser
    (models/yolo.py:1523-1535) but ships no yaml that names them.  The rows keep their arguments and n: CNeB repeats its blocks inside; the
    parser does not insert n for CSPCM, so n > 1 there is n whole modules in a row - legal here, where every swapped row has c1 == c2.  The
    head and Detect are yolov5_cfg's."""
    if where not in CONVNEXT_WHERE:
        raise ValueError(f'where must be one of {tuple(CONVNEXT_WHERE)}, got {where!r}')
    cfg = yolov5_cfg(width, depth, nc, anchors)
    for row in cfg['backbone']:
        if row[2] == 'C3':
            row[2] = CONVNEXT_WHERE[where]
    return cfg


def yolov5_swin_cfg(width=0.50, depth=0.33, nc=80, anchors=None):
    """The layer table of models/hub/yolov5s-transformer.yaml (yolov5s with the Focus stem and SPP(5,9,13), a transformer C3 as the last
    backbone row) with C3STR - the Swin variant, models/common.py:1632-1637 - where that file has C3TR (row 9).  The reference registers C3STR
    in its parser (models/yolo.py:1476,1487) but ships no yaml that names it; C3TR itself stays outside the path.  Defaults are the yaml's."""
    cfg = yolov5_cfg(width, depth, nc, anchors, version='5.0')
    cfg['backbone'][9][2] = 'C3STR'
    return cfg


def yolov5_ca_cfg(width=0.50, depth=0.33, nc=80, anchors=None, where='c3'):
    """yolov5s 6.0 with coordinate attention (models/common.py:1399-1450, 4884-4931).  The reference registers C3_CA and CoorAttention in its
    parser (models/yolo.py:1477, 1630-1634) but ships no yaml that names them.  where='c3': the four backbone C3 rows become C3_CA - which the
    reference does not repeat inside, so the rows with n > 1 are n whole blocks in a row; where='row': a [-1, 1, 'CoorAttention', [1024]] row
    behind SPPF, the head's absolute indices one up."""
    if where not in ('c3', 'row'):
        raise ValueError(f"where must be 'c3' or 'row', got {where!r}")
    cfg = yolov5_cfg(width, depth, nc, anchors)
    if where == 'c3':
        for row in cfg['backbone']:
            if row[2] == 'C3':
                row[2] = 'C3_CA'
        return cfg
    cfg['backbone'].append([-1, 1, 'CoorAttention', [1024]])
    for row in cfg['head']:
        if isinstance(row[0], list):
            row[0] = [j + 1 if j >= 10 else j for j in row[0]]
    return cfg


def yolov5_ema_cfg(width=0.50, depth=0.33, nc=80, anchors=None, where='c2f'):
    """yolov5s 6.0 with efficient multi-scale attention (EMA, models/common.py:5263-5292; iRMB_EMA, iRMB_EMABottleneck and C2f_iRMB_EMA,
    :5409-5497).  The reference's parser registers none of them: its generic branch builds them from the yaml arguments as written and records the
    input's width (models/yolo.py:1648-1650), and it ships no yaml that names them.  where='c2f': the four backbone C3 rows become
    [-1, 1, 'C2f_iRMB_EMA', [c, c, n, True]] with c and n written out already scaled, since that branch scales nothing; where='row': an
    [-1, 1, 'EMA', [c]] row behind SPPF, c the scaled width there, the head's absolute indices one up."""
    if where not in ('c2f', 'row'):
        raise ValueError(f"where must be 'c2f' or 'row', got {where!r}")
    cfg = yolov5_cfg(width, depth, nc, anchors)
    scaled = lambda c: math.ceil(c * width / 8) * 8              # noqa: E731  (make_divisible(c * gw, 8), models/yolo.py:1481)
    if where == 'c2f':
        for row in cfg['backbone']:
            if row[2] == 'C3':
                n = max(round(row[1] * depth), 1) if row[1] > 1 else row[1]
                row[1:] = [1, 'C2f_iRMB_EMA', [scaled(row[3][0]), scaled(row[3][0]), n, True]]
        return cfg
    cfg['backbone'].append([-1, 1, 'EMA', [scaled(1024)]])
    for row in cfg['head']:
        if isinstance(row[0], list):
            row[0] = [j + 1 if j >= 10 else j for j in row[0]]
    return cfg


def yolov5_acmix_cfg(width=0.50, depth=0.33, nc=80, anchors=None, where='row'):
    """yolov5s 6.0 with ACmix (models/common.py:7281-7365), which the reference registers in its parser with a scaled width (models/yolo.py:
    1496-1501) but names in no yaml it ships.  where='row': a [-1, 1, 'ACmix', [1024]] row behind SPPF as row 10, the head's absolute indices
    one up; where='p3': a [-1, 1, 'ACmix', [256]] row behind the P3 head C3 (row 17) as row 18 - the rows behind it move one down, the next Conv
    reads the new row and Detect reads [18, 21, 24]."""
    if where not in ('row', 'p3'):
        raise ValueError(f"where must be 'row' or 'p3', got {where!r}")
    cfg = yolov5_cfg(width, depth, nc, anchors)
    if where == 'row':
        cfg['backbone'].append([-1, 1, 'ACmix', [1024]])
        for row in cfg['head']:
            if isinstance(row[0], list):
                row[0] = [j + 1 if j >= 10 else j for j in row[0]]
        return cfg
    at = 18 - len(cfg['backbone'])                                # head position of the new row 18
    cfg['head'].insert(at, [-1, 1, 'ACmix', [256]])
    for row in cfg['head'][at + 1:]:
        if isinstance(row[0], list):
            row[0] = [j + 1 if j >= 17 else j for j in row[0]]
    return cfg


def yolov5_context_cfg(width=0.50, depth=0.33, nc=80, anchors=None, where='aspp'):
    """yolov5s 6.0 with the dilated-convolution context blocks (ASPP, models/common.py:1829-1843; C2f_DWR, :7431-7511).  The reference registers
    both in its parser (models/yolo.py:1472-1492, C2f_DWR among the modules repeated inside) but ships no yaml that names them.  where='aspp': a
    [-1, 1, 'ASPP', [1024]] row in SPPF's place; where='dwr': [-1, n, 'C2f_DWR', [512, True]] and [-1, n, 'C2f_DWR', [1024, True]] in place of
    the P4 and P5 backbone C3 rows, same n; where='both': both changes."""
    if where not in ('aspp', 'dwr', 'both'):
        raise ValueError(f"where must be 'aspp', 'dwr' or 'both', got {where!r}")
    cfg = yolov5_cfg(width, depth, nc, anchors)
    bb = cfg['backbone']
    if where in ('aspp', 'both'):
        (i,) = [j for j, row in enumerate(bb) if row[2] == 'SPPF']
        bb[i] = [-1, 1, 'ASPP', [1024]]
    if where in ('dwr', 'both'):
        for j, row in enumerate(bb):
            if row[2] == 'C3' and row[3][0] in (512, 1024):
                bb[j] = [row[0], row[1], 'C2f_DWR', [row[3][0], True]]
    return cfg


def yolov5_cpca_cfg(width=0.50, depth=0.33, nc=80, anchors=None, where='c3'):
    """yolov5s 6.0 with channel prior convolutional attention (models/common.py:5753-5859, 1684-1689).  The reference registers C3CPCA and CPCA
    in its parser (models/yolo.py:1477, 1490, 1566-1568) but ships no yaml that names them.  where='c3': the four backbone C3 rows become
    C3CPCA, repeated inside like C3; where='row': a [-1, 1, 'CPCA', []] row behind SPPF (sized by its input), the head's absolute indices
    one up."""
    if where not in ('c3', 'row'):
        raise ValueError(f"where must be 'c3' or 'row', got {where!r}")
    cfg = yolov5_cfg(width, depth, nc, anchors)
    if where == 'c3':
        for row in cfg['backbone']:
            if row[2] == 'C3':
                row[2] = 'C3CPCA'
        return cfg
    cfg['backbone'].append([-1, 1, 'CPCA', []])
    for row in cfg['head']:
        if isinstance(row[0], list):
            row[0] = [j + 1 if j >= 10 else j for j in row[0]]
    return cfg


CBAM_VARIANTS = {'cbam': 'C3_CBAM', 'cbams': 'C3_CBAMS', 'cbam_dwc': 'C3_CBAM_DWC', 'cbams_dwc': 'C3_CBAMS_DWC', 'scbam': 'C3_SCBAM', 'row': 'C3CBAM'}


def yolov5_cbam_cfg(width=0.50, depth=0.33, nc=80, anchors=None, variant='cbam'):
    """yolov5s 6.0 with the CBAM C3 family (models/common.py:494-504, 1640-1705).  The reference registers the names in its parser
    (models/yolo.py:1473-1477, 1487-1490) but ships no yaml that names them.  variant 'cbam' / 'cbams' / 'cbam_dwc' / 'cbams_dwc' / 'scbam': the
    four backbone C3 rows become C3_CBAM / C3_CBAMS / C3_CBAM_DWC / C3_CBAMS_DWC / C3_SCBAM, repeated inside like C3; 'row': a
    [-1, 1, 'C3CBAM', [1024]] row behind SPPF (it must name its input's width, which it passes through), the head's absolute indices one up."""
    if variant not in CBAM_VARIANTS:
        raise ValueError(f'variant must be one of {tuple(CBAM_VARIANTS)}, got {variant!r}')
    cfg = yolov5_cfg(width, depth, nc, anchors)
    if variant != 'row':
        for row in cfg['backbone']:
            if row[2] == 'C3':
                row[2] = CBAM_VARIANTS[variant]
        return cfg
    cfg['backbone'].append([-1, 1, 'C3CBAM', [1024]])
    for row in cfg['head']:
        if isinstance(row[0], list):
            row[0] = [j + 1 if j >= 10 else j for j in row[0]]
    return cfg


SIMAM_WHERE = ('row', 'slicing', 'sws', 'ps')


def yolov5_simam_cfg(width=0.50, depth=0.33, nc=80, anchors=None, where='row'):
    """yolov5s 6.0 with the parameter-free SimAM attention family (models/common.py:2915-2961, 9374-9495).  The reference registers the five
    names in its parser (models/yolo.py:1472, 1502-1513 and the generic branch) but ships no yaml that names them.  where='row': a
    [-1, 1, 'SimAM', [1024]] row behind SPPF; 'slicing': a [-1, 1, 'SimAMWithSlicing', [1024]] row there; 'ps': a PSSimAM row there, its
    arguments - used as written by the parser - the width-scaled channel count; for these three the head's absolute indices move one up.
    'sws': the P3 and P4 stride-2 backbone Convs (rows 3 and 5) become Conv_SWS [c2, 8, 0.5, 1e-4, 3, 2]: 8 x 8 windows at stride 4."""
    if where not in SIMAM_WHERE:
        raise ValueError(f'where must be one of {SIMAM_WHERE}, got {where!r}')
    cfg = yolov5_cfg(width, depth, nc, anchors)
    if where == 'sws':
        for i in (3, 5):
            row = cfg['backbone'][i]
            row[2], row[3] = 'Conv_SWS', [row[3][0], 8, 0.5, 1e-4, 3, 2]
        return cfg
    c = math.ceil(1024 * width / 8) * 8                           # the parser's make_divisible(1024 * width, 8)
    cfg['backbone'].append({'row': [-1, 1, 'SimAM', [1024]], 'slicing': [-1, 1, 'SimAMWithSlicing', [1024]], 'ps': [-1, 1, 'PSSimAM', [c, c]]}[where])
    for row in cfg['head']:
        if isinstance(row[0], list):
            row[0] = [j + 1 if j >= 10 else j for j in row[0]]
    return cfg


def yolov5_ghost_cfg(width=0.50, depth=0.33, nc=80, anchors=None):
    """The layer table of models/hub/yolov5s-ghost.yaml as a dict: yolov5s with GhostConv for the strided and lateral convs and C3Ghost for
    C3 (Focus stem, SPP(5,9,13)).  Defaults are the yaml's (depth 0.33, width 0.50, 80 classes, the COCO anchors)."""
    import copy
    bb = [[-1, 1, 'Focus', [64, 3]], [-1, 1, 'GhostConv', [128, 3, 2]], [-1, 3, 'C3Ghost', [128]], [-1, 1, 'GhostConv', [256, 3, 2]],
          [-1, 9, 'C3Ghost', [256]], [-1, 1, 'GhostConv', [512, 3, 2]], [-1, 9, 'C3Ghost', [512]], [-1, 1, 'GhostConv', [1024, 3, 2]],
          [-1, 1, 'SPP', [1024, [5, 9, 13]]], [-1, 3, 'C3Ghost', [1024, False]]]
    up = [-1, 1, 'nn.Upsample', [None, 2, 'nearest']]
    hd = [[-1, 1, 'GhostConv', [512, 1, 1]], up, [[-1, 6], 1, 'Concat', [1]], [-1, 3, 'C3Ghost', [512, False]],
          [-1, 1, 'GhostConv', [256, 1, 1]], up, [[-1, 4], 1, 'Concat', [1]], [-1, 3, 'C3Ghost', [256, False]],
          [-1, 1, 'GhostConv', [256, 3, 2]], [[-1, 14], 1, 'Concat', [1]], [-1, 3, 'C3Ghost', [512, False]],
          [-1, 1, 'GhostConv', [512, 3, 2]], [[-1, 10], 1, 'Concat', [1]], [-1, 3, 'C3Ghost', [1024, False]],
          [[17, 20, 23], 1, 'Detect', ['nc', 'anchors']]]
    return dict(nc=nc, depth_multiple=depth, width_multiple=width, anchors=copy.deepcopy(anchors or COCO_ANCHORS),
                backbone=copy.deepcopy(bb), head=copy.deepcopy(hd))


def yolov10_cfg(width=1.0, depth=1.0, nc=10, anchors=None, upsample='nearest'):
    """The layer table of models/hub/yolov10.yaml as a dict: Conv / C2f / SCDown backbone, C2fCIB at P5, SPPF, PSA, a C2f / C2fCIB PAN head
    and the plain Detect.  Defaults are the yaml's (depth 1.0, width 1.0, 10 classes).  anchors=None gives the COCO anchors: the yaml's
    `anchors: 3` is a placeholder (list(range(6)) per level) that only makes sense after autoanchor; anchors=3 reproduces the yaml exactly -
    `somi_amd.autoanchor.check_anchors(dataset, model)` then replaces the placeholder from the data set's labels.
    upsample='carafe' | 'dysample': the head's two nn.Upsample rows become the learned upsampler (UPSAMPLE_ROWS)."""
    import copy
    bb = [[-1, 1, 'Conv', [64, 3, 2]], [-1, 1, 'Conv', [128, 3, 2]], [-1, 3, 'C2f', [128, True]], [-1, 1, 'Conv', [256, 3, 2]],
          [-1, 6, 'C2f', [256, True]], [-1, 1, 'SCDown', [512, 3, 2]], [-1, 6, 'C2f', [512, True]], [-1, 1, 'SCDown', [1024, 3, 2]],
          [-1, 3, 'C2fCIB', [1024, True]], [-1, 1, 'SPPF', [1024, 5]], [-1, 1, 'PSA', [1024]]]
    up = [-1, 1, 'nn.Upsample', [None, 2, 'nearest']]
    hd = [up, [[-1, 6], 1, 'Concat', [1]], [-1, 3, 'C2fCIB', [512, True]],
          up, [[-1, 4], 1, 'Concat', [1]], [-1, 3, 'C2f', [256]],
          [-1, 1, 'Conv', [256, 3, 2]], [[-1, 13], 1, 'Concat', [1]], [-1, 3, 'C2fCIB', [512, True]],
          [-1, 1, 'SCDown', [512, 3, 2]], [[-1, 10], 1, 'Concat', [1]], [-1, 3, 'C2fCIB', [1024, True]],
          [[16, 19, 22], 1, 'Detect', ['nc', 'anchors']]]
    anchors = COCO_ANCHORS if anchors is None else anchors
    return dict(nc=nc, depth_multiple=depth, width_multiple=width, anchors=copy.deepcopy(anchors),
                backbone=copy.deepcopy(bb), head=_swap_upsample(copy.deepcopy(hd), upsample))


YOLOV3_TINY_ANCHORS = [[10, 14, 23, 27, 37, 58], [81, 82, 135, 169, 344, 319]]
"""The P4 / P5 anchors of models/hub/yolov3-tiny.yaml."""


def yolov3_cfg(variant='', width=1.0, depth=1.0, nc=80, anchors=None):
    """The layer tables of models/hub/yolov3.yaml (variant ''), yolov3-spp.yaml ('spp': SPP(5, 9, 13) in place of the head's first 1x1 Conv) and
    yolov3-tiny.yaml ('tiny': Conv / nn.MaxPool2d backbone, nn.ZeroPad2d + stride-1 pool, two Detect levels) as dicts.  Defaults are the yamls'
    (depth 1.0, width 1.0, 80 classes, their own anchors).  The Darknet-53 stages repeat Bottleneck 2 / 8 / 8 / 4 times as nn.Sequentials."""
    import copy
    up = [-1, 1, 'nn.Upsample', [None, 2, 'nearest']]
    if variant == 'tiny':
        mp = [-1, 1, 'nn.MaxPool2d', [2, 2, 0]]
        bb = [[-1, 1, 'Conv', [16, 3, 1]], mp, [-1, 1, 'Conv', [32, 3, 1]], mp, [-1, 1, 'Conv', [64, 3, 1]], mp, [-1, 1, 'Conv', [128, 3, 1]], mp,
              [-1, 1, 'Conv', [256, 3, 1]], mp, [-1, 1, 'Conv', [512, 3, 1]], [-1, 1, 'nn.ZeroPad2d', [[0, 1, 0, 1]]],
              [-1, 1, 'nn.MaxPool2d', [2, 1, 0]]]
        hd = [[-1, 1, 'Conv', [1024, 3, 1]], [-1, 1, 'Conv', [256, 1, 1]], [-1, 1, 'Conv', [512, 3, 1]], [-2, 1, 'Conv', [128, 1, 1]], up,
              [[-1, 8], 1, 'Concat', [1]], [-1, 1, 'Conv', [256, 3, 1]], [[19, 15], 1, 'Detect', ['nc', 'anchors']]]
        default = YOLOV3_TINY_ANCHORS
    elif variant in ('', 'spp'):
        bb = [[-1, 1, 'Conv', [32, 3, 1]], [-1, 1, 'Conv', [64, 3, 2]], [-1, 1, 'Bottleneck', [64]], [-1, 1, 'Conv', [128, 3, 2]],
              [-1, 2, 'Bottleneck', [128]], [-1, 1, 'Conv', [256, 3, 2]], [-1, 8, 'Bottleneck', [256]], [-1, 1, 'Conv', [512, 3, 2]],
              [-1, 8, 'Bottleneck', [512]], [-1, 1, 'Conv', [1024, 3, 2]], [-1, 4, 'Bottleneck', [1024]]]
        second = [-1, 1, 'SPP', [512, [5, 9, 13]]] if variant == 'spp' else [-1, 1, 'Conv', [512, [1, 1]]]
        hd = [[-1, 1, 'Bottleneck', [1024, False]], second, [-1, 1, 'Conv', [1024, 3, 1]], [-1, 1, 'Conv', [512, 1, 1]],
              [-1, 1, 'Conv', [1024, 3, 1]], [-2, 1, 'Conv', [256, 1, 1]], up, [[-1, 8], 1, 'Concat', [1]],
              [-1, 1, 'Bottleneck', [512, False]], [-1, 1, 'Bottleneck', [512, False]], [-1, 1, 'Conv', [256, 1, 1]],
              [-1, 1, 'Conv', [512, 3, 1]], [-2, 1, 'Conv', [128, 1, 1]], up, [[-1, 6], 1, 'Concat', [1]],
              [-1, 1, 'Bottleneck', [256, False]], [-1, 2, 'Bottleneck', [256, False]], [[27, 22, 15], 1, 'Detect', ['nc', 'anchors']]]
        default = COCO_ANCHORS
    else:
        raise ValueError(f"yolov3_cfg: variant {variant!r} (one of '', 'spp', 'tiny')")
    return dict(nc=nc, depth_multiple=depth, width_multiple=width, anchors=copy.deepcopy(default if anchors is None else anchors),
                backbone=copy.deepcopy(bb), head=copy.deepcopy(hd))


def yolov5_hub_cfg(name, width=1.0, depth=1.0, nc=80, anchors=None):
    """The layer tables of models/hub/yolov5-fpn.yaml ('fpn': Bottleneck x3 as an nn.Sequential, BottleneckCSP, top-down head only),
    yolov5-panet.yaml ('panet': BottleneckCSP everywhere), yolov5-p6.yaml ('p6': C3, SPP(3, 5, 7), Detect over P3..P6) and yolov5-p7.yaml ('p7': C3,
    SPP(3, 5), Detect over P3..P7) as dicts.  Defaults are the yamls' (depth 1.0, width 1.0, 80 classes; the COCO anchors for fpn / panet, and for
    p6 / p7 the yamls' `anchors: 3`, a placeholder of list(range(6)) per level that only makes sense after autoanchor - pass real ones, or run
    `somi_amd.autoanchor.check_anchors(dataset, model)` on the built model)."""
    import copy
    up = [-1, 1, 'nn.Upsample', [None, 2, 'nearest']]

    def cat(j):
        return [[-1, j], 1, 'Concat', [1]]
    if name == 'fpn':
        bb = [[-1, 1, 'Focus', [64, 3]], [-1, 1, 'Conv', [128, 3, 2]], [-1, 3, 'Bottleneck', [128]], [-1, 1, 'Conv', [256, 3, 2]],
              [-1, 9, 'BottleneckCSP', [256]], [-1, 1, 'Conv', [512, 3, 2]], [-1, 9, 'BottleneckCSP', [512]], [-1, 1, 'Conv', [1024, 3, 2]],
              [-1, 1, 'SPP', [1024, [5, 9, 13]]], [-1, 6, 'BottleneckCSP', [1024]]]
        hd = [[-1, 3, 'BottleneckCSP', [1024, False]], up, cat(6), [-1, 1, 'Conv', [512, 1, 1]], [-1, 3, 'BottleneckCSP', [512, False]],
              up, cat(4), [-1, 1, 'Conv', [256, 1, 1]], [-1, 3, 'BottleneckCSP', [256, False]], [[18, 14, 10], 1, 'Detect', ['nc', 'anchors']]]
        default = COCO_ANCHORS
    elif name == 'panet':
        bb = [[-1, 1, 'Focus', [64, 3]], [-1, 1, 'Conv', [128, 3, 2]], [-1, 3, 'BottleneckCSP', [128]], [-1, 1, 'Conv', [256, 3, 2]],
              [-1, 9, 'BottleneckCSP', [256]], [-1, 1, 'Conv', [512, 3, 2]], [-1, 9, 'BottleneckCSP', [512]], [-1, 1, 'Conv', [1024, 3, 2]],
              [-1, 1, 'SPP', [1024, [5, 9, 13]]], [-1, 3, 'BottleneckCSP', [1024, False]]]
        hd = [[-1, 1, 'Conv', [512, 1, 1]], up, cat(6), [-1, 3, 'BottleneckCSP', [512, False]],
              [-1, 1, 'Conv', [256, 1, 1]], up, cat(4), [-1, 3, 'BottleneckCSP', [256, False]],
              [-1, 1, 'Conv', [256, 3, 2]], cat(14), [-1, 3, 'BottleneckCSP', [512, False]],
              [-1, 1, 'Conv', [512, 3, 2]], cat(10), [-1, 3, 'BottleneckCSP', [1024, False]], [[17, 20, 23], 1, 'Detect', ['nc', 'anchors']]]
        default = COCO_ANCHORS
    elif name in ('p6', 'p7'):
        wide = [128, 256, 512, 768, 1024] + ([1280] if name == 'p7' else [])       # P2 .. P6 / P7
        reps = [3, 9, 9, 3] + ([3] if name == 'p7' else [])
        bb = [[-1, 1, 'Focus', [64, 3]]]
        for c, n in zip(wide[:-1], reps):
            bb += [[-1, 1, 'Conv', [c, 3, 2]], [-1, n, 'C3', [c]]]
        bb += [[-1, 1, 'Conv', [wide[-1], 3, 2]], [-1, 1, 'SPP', [wide[-1], [3, 5, 7] if name == 'p6' else [3, 5]]],
               [-1, 3, 'C3', [wide[-1], False]]]
        nb, hd = len(bb), []
        lateral = []                                              # indices of the top-down 1x1 Convs, coarsest first
        for j, c in enumerate(reversed(wide[1:-1])):              # top-down: 1x1, upsample, cat the backbone level below, C3
            lateral.append(nb + len(hd))
            hd += [[-1, 1, 'Conv', [c, 1, 1]], up, cat(nb - 3 - 2 * j - 1), [-1, 3, 'C3', [c, False]]]
        outs = [nb + len(hd) - 1]
        for c, nxt, lat in zip(wide[1:-1], wide[2:], reversed(lateral)):            # bottom-up: 3x3 / 2, cat the lateral, C3
            hd += [[-1, 1, 'Conv', [c, 3, 2]], cat(lat), [-1, 3, 'C3', [nxt, False]]]
            outs.append(nb + len(hd) - 1)
        hd.append([outs, 1, 'Detect', ['nc', 'anchors']])
        default = 3
    else:
        raise ValueError(f"yolov5_hub_cfg: name {name!r} (one of 'fpn', 'panet', 'p6', 'p7')")
    return dict(nc=nc, depth_multiple=depth, width_multiple=width, anchors=copy.deepcopy(default if anchors is None else anchors),
                backbone=copy.deepcopy(bb), head=copy.deepcopy(hd))


def tiny_somi_cfg(nc=10):
    """A cut-down graph that uses every module class of the SOMI yaml once (Conv, ODConv_3rd, C2fCBAM, SPPF, nn.Upsample, BiFPN, SEAM,
    DecoupledDetect) at 32 / 64 channels, two detection levels: ~0.2 M parameters - for fixtures that carry whole pickled models."""
    import copy
    bb = [[-1, 1, 'Conv', [32, 3, 2]], [-1, 1, 'ODConv_3rd', [32, 3, 2, 4]], [-1, 1, 'C2fCBAM', [32, True]], [-1, 1, 'Conv', [64, 3, 2]],
          [-1, 1, 'SPPF', [64, 5]]]
    hd = [[2, 1, 'Conv', [32]], [4, 1, 'Conv', [32]], [-1, 1, 'nn.Upsample', [None, 2, 'nearest']], [[-1, 5], 1, 'BiFPN', []],
          [-1, 1, 'SEAM', [32, 1, 16]], [-1, 1, 'C2fCBAM', [32]], [[10, 6], 1, 'DecoupledDetect', ['nc', 'anchors']]]
    return dict(nc=nc, depth_multiple=1.0, width_multiple=1.0, anchors=[[4, 6, 12, 8, 7, 14, 20, 12], [13, 22, 31, 18, 21, 33, 46, 23]],
                backbone=copy.deepcopy(bb), head=copy.deepcopy(hd))
