"""Scene builders for the NMS stage-boundary tests (test infrastructure, CPU torch only): inputs whose few hundred output rows show what
the count / scan / emit, the top-30000 select, the order-preserving compaction, the rank sort and the greedy rounds decided at their own
boundaries.  tests/test_nms_edges_host.py proves on the CPU that each scene shows its decision; tests/test_nms_edges_gpu.py runs them.

Sites and witnesses.  Boxes sit on a lattice of sites (a 16 px box every 32 px, or 12 px every 20 px): two boxes on one site are identical
(IoU 1: the lower ranked one goes under every rule), boxes on different sites are disjoint (IoU 0, the penalised metrics negative:
nothing goes).  All coordinates are small integers and halves, so this is exact in fp32.  A witness is a candidate alone on a site of its
own: it is in the output iff the stage under test selected it, which makes a decision at rank ~30000 visible in the output's head.

Ranks, tie ranks and candidate indices are computed from the finished scene.
"""
import functools

import numpy as np
import torch

from oracle.somi_ref import nms as O

import nms_variants_ref as R

MAX_NMS = 30000                 # utils/general.py:641
SEL_CHUNK = 4096                # candidates per select workgroup
SCAN_WIDTH = 256                # chunks one pass of either prefix scan covers
U16 = 2.0 ** -16


def site_xywh(site, box=16.0, pitch=32.0, per_row=18):
    """(n, 4) centre/size boxes of lattice sites."""
    site = torch.as_tensor(site, dtype=torch.long)
    out = torch.empty(site.numel(), 4)
    out[:, 0] = (site % per_row).float() * pitch + pitch / 2
    out[:, 1] = (site // per_row).float() * pitch + pitch / 2
    out[:, 2:] = box
    return out


def site_xyxy(site, **kw):
    return O.xywh2xyxy(site_xywh(site, **kw))


def has_site(out, site, **kw):
    """Is there an output row on this site?"""
    xy = site_xyxy([site], **kw)[0]
    return bool((out[:, :4] == xy).all(1).any())


# ------------------------------------------------------------------------------------------------ the pipeline, stage by stage
def candidates(img, conf_thres, multi_label=False):
    """One image's candidate rows [x1, y1, x2, y2, conf, cls] in emission order, built as the oracle builds them, and the prediction row
    each one came from."""
    nc = img.shape[1] - 5
    live = img[:, 4] > conf_thres
    rows = live.nonzero().view(-1)
    x = img[live].clone()
    x[:, 5:] *= x[:, 4:5]
    box = O.xywh2xyxy(x[:, :4])
    if multi_label and nc > 1:
        i, j = (x[:, 5:] > conf_thres).nonzero(as_tuple=False).T
        return torch.cat((box[i], x[i, j + 5, None], j[:, None].float()), 1), rows[i]
    conf, j = x[:, 5:].max(1, keepdim=True)
    m = conf.view(-1) > conf_thres
    return torch.cat((box, conf, j.float()), 1)[m], rows[m]


def select(scores, take=MAX_NMS, ties_descending=False):
    """Indices of the first `take` candidates by (score descending, index ascending); ties_descending=True is the wrong tie rule."""
    s = scores.numpy()
    if ties_descending:
        order = np.lexsort((-np.arange(s.size), -s))
    else:
        order = np.argsort(-s, kind='stable')
    return torch.from_numpy(order[:take].copy())


def finish(x, order, iou_thres, max_det=300):
    """The selected candidates in rank order -> output rows: class offset, greedy NMS, the max_det cut."""
    x = x[order]
    keep = O.greedy_nms(x[:, :4] + x[:, 5:6] * 4096, x[:, 4], iou_thres)
    return x[keep[:max_det]]


def emit_without_carry(x, rows, chunk_rows):
    """The candidate list a count scan gives that restarts its offsets at every SCAN_WIDTH-th chunk: each group of chunks writes from
    slot 0, the last group's count is the total."""
    group = torch.div(rows, chunk_rows * SCAN_WIDTH, rounding_mode='floor')
    slots = torch.full((x.shape[0],), -1, dtype=torch.long)
    total = 0
    for gi in range(int(group.max()) + 1):
        idx = (group == gi).nonzero().view(-1)
        slots[:idx.numel()] = idx
        total = idx.numel()
    return x[slots[:total]]


def select_without_carry(scores):
    """The compaction's survivors if the scan over select chunks restarted at every SCAN_WIDTH-th chunk (prefixes of `key < T` and of
    `key == T` both): later groups write from slot 0 and count their ties from 0; slots nobody wrote are dropped.  In rank order."""
    n = scores.numel()
    ranked = select(scores, n)
    T = scores[ranked[MAX_NMS - 1]]
    r = MAX_NMS - int((scores > T).sum())
    slots = torch.full((MAX_NMS,), -1, dtype=torch.long)
    for g0 in range(0, n, SEL_CHUNK * SCAN_WIDTH):
        idx = torch.arange(g0, min(g0 + SEL_CHUNK * SCAN_WIDTH, n))
        s = scores[idx]
        lt, eq = (s > T).long(), (s == T).long()
        lt_rank, eq_rank = lt.cumsum(0) - lt, eq.cumsum(0) - eq
        sel = (lt == 1) | ((eq == 1) & (eq_rank < r))
        slots[(lt_rank + eq_rank.clamp(max=r))[sel]] = idx[sel]
    cand = slots[slots >= 0]
    return cand[select(scores[cand], MAX_NMS)]


# ------------------------------------------------------------------------------------------------ scenes 1, 2, 6: a tie across the cut
def tie_layout(n, nc, seed, base_sites, tie_rows=None, ranks=None, borders=(), low_witnesses=0, n_high=28500, n_tie=3000):
    """(n, 5 + nc) rows with objectness 1 whose n * nc class scores are n_high distinct values in (0.5, 1), n_tie cells at exactly 0.5 (one
    per row at most) and the rest in (0.3, 0.49): the cut at 30000 falls inside the tie, r = 30000 - n_high of them are taken, in
    candidate order.  The tied cells at the tie ranks `ranks(r)`, and the last one before / first one at or after every candidate index
    in `borders`, are witnesses: the row keeps that class alone (the others 0) and moves to a site of its own; the distinct scores its
    cleared cells held move to cells of the lower group, so n_high and the tie ranks stand.  `low_witnesses` rows (nc = 1) of the lower
    group get sites of their own too.  -> (rows, meta)."""
    g = torch.Generator().manual_seed(seed)
    r = MAX_NMS - n_high
    if tie_rows is None:
        tie_rows = torch.randperm(n, generator=g)[:n_tie]
    tie_rows = tie_rows.sort().values
    assert tie_rows.numel() == n_tie == tie_rows.unique().numel()
    tie_cls = torch.randint(0, nc, (n_tie,), generator=g)
    score = torch.zeros(n, nc)
    flat = score.view(-1)
    tie_cell = tie_rows * nc + tie_cls                               # ascending: the candidate order of the tie
    is_tie = torch.zeros(n * nc, dtype=torch.bool)
    is_tie[tie_cell] = True
    free = (~is_tie).nonzero().view(-1)
    free = free[torch.randperm(free.numel(), generator=g)]
    high, low = free[:n_high], free[n_high:]
    flat[high] = (0.5 + (torch.arange(n_high, dtype=torch.float64) + 1) * U16).float()
    flat[low] = (0.3 + ((torch.arange(low.numel(), dtype=torch.float64) % 8192) + 1) * U16).float()
    flat[tie_cell] = 0.5

    def tie_index(wit):
        """candidate index of every tied cell when the tie ranks `wit` are witnesses"""
        live = torch.ones(n, nc, dtype=torch.bool)
        w = torch.tensor(sorted(wit), dtype=torch.long)
        live[tie_rows[w]] = False
        live[tie_rows[w], tie_cls[w]] = True
        return (live.view(-1).cumsum(0) - 1)[tie_cell]

    wit = set(int(k) % n_tie for k in (ranks(r) if ranks else ()))
    for m in borders:                                                # ascending; a new witness row moves what follows it only
        while True:
            idx = tie_index(wit)
            before, after = int((idx < m).sum()) - 1, int((idx < m).sum())
            pair = {k for k in (before, after) if 0 <= k < n_tie}
            if pair <= wit:
                break
            wit |= pair
    wit = sorted(wit)
    w = torch.tensor(wit, dtype=torch.long)
    wrow = torch.zeros(n, dtype=torch.bool)
    wrow[tie_rows[w]] = True
    low = low[~wrow[torch.div(low, nc, rounding_mode='floor')]]      # lower-group cells outside the witness rows
    lost = flat[high[wrow[torch.div(high, nc, rounding_mode='floor')]]].clone()
    flat[low[:lost.numel()]] = lost
    low = low[lost.numel():]
    keep = flat[tie_cell[w]].clone()
    score[tie_rows[w]] = 0
    flat[tie_cell[w]] = keep
    site = torch.randint(0, base_sites, (n,), generator=g)
    site[tie_rows[w]] = base_sites + torch.arange(len(wit))
    low_rows = torch.zeros(0, dtype=torch.long)
    if low_witnesses:
        assert nc == 1
        low_rows = low[:low_witnesses]
        site[low_rows] = base_sites + len(wit) + torch.arange(low_witnesses)
    rows = torch.zeros(n, 5 + nc)
    rows[:, :4] = site_xywh(site)
    rows[:, 4] = 1.0
    rows[:, 5:] = score
    meta = dict(r=r, tie_rows=tie_rows, tie_cls=tie_cls, tie_index=tie_index(wit), witness_ranks=wit, witness_sites=site[tie_rows[w]].tolist(),
                low_sites=site[low_rows].tolist(), n_sites=base_sites + len(wit) + low_witnesses)
    return rows, meta


def ranked_layout(n, scores_by_rank, witness_ranks, seed, base_sites=150):
    """(n, 6) rows, nc = 1: a random len(scores_by_rank) of them are candidates (objectness 1, the others 0) and hold the given scores
    (descending) in random order; the candidates at `witness_ranks` of the finished scene's stable ranking get sites of their own."""
    g = torch.Generator().manual_seed(seed)
    k = scores_by_rank.numel()
    cand = torch.randperm(n, generator=g)[:k].sort().values
    score = torch.empty(k)
    score[torch.randperm(k, generator=g)] = scores_by_rank
    order = select(score, k)
    site = torch.randint(0, base_sites, (n,), generator=g)
    wrows = cand[order[torch.tensor(list(witness_ranks))]]
    site[wrows] = base_sites + torch.arange(len(witness_ranks))
    rows = torch.zeros(n, 6)
    rows[:, :4] = site_xywh(site)
    rows[cand, 4] = 1.0
    rows[:, 5] = 0.9                                                  # a row without objectness must not get in on its class score
    rows[cand, 5] = score
    index = torch.full((n,), -1, dtype=torch.long)
    index[cand] = torch.arange(k)
    meta = dict(witness_ranks=list(witness_ranks), witness_sites=site[wrows].tolist(), witness_index=index[wrows].tolist(),
                n_sites=base_sites + len(witness_ranks), n_cand=k)
    return rows, meta


def _bits(b):
    return torch.from_numpy(np.asarray(b, dtype=np.int64).astype(np.uint32).view(np.float32).copy())


CUT_KINDS = ('ties', 'ulp', 'mid', 'exact', 'plus1')
CUT_KW = dict(conf_thres=0.25, iou_thres=0.45)
CUT_N, CUT_LIVE1 = 36000, 29000


@functools.lru_cache(maxsize=None)
def cut_scene(kind):
    """Scene 1 -> ((3, 36000, 6) predictions, meta of image 0).  Image 1: the same rows with objectness 0 from row 29000 on (at most 30000
    candidates: no select); image 2: no candidates."""
    n = CUT_N
    if kind == 'ties':
        borders = list(range(SEL_CHUNK, n, SEL_CHUNK))
        img, meta = tie_layout(n, 1, 101, 150, ranks=lambda r: (0, 1, r - 2, r - 1, r, r + 1, -1), borders=borders, low_witnesses=5)
    elif kind in ('ulp', 'mid'):
        step = 1 if kind == 'ulp' else 256                           # 1: only the level-3 histogram separates neighbours; 256: level 2
        top = (0.7 + (25000 - torch.arange(25000, dtype=torch.float64)) * 2.0 ** -17).float()
        rest = _bits(0x3F000000 + step * (10999 - np.arange(11000)))
        img, meta = ranked_layout(n, torch.cat((top, rest)), range(MAX_NMS - 8, MAX_NMS + 8), 102 if kind == 'ulp' else 103)
    elif kind == 'exact':                                            # exactly 30000 candidates: nothing to select
        s = (0.3 + (MAX_NMS - torch.arange(MAX_NMS, dtype=torch.float64)) * U16).float()
        img, meta = ranked_layout(n, s, range(MAX_NMS - 4, MAX_NMS), 104)
    else:                                                            # 30001: the one dropped is the last of a tie of four
        s = (0.3 + (MAX_NMS + 1 - torch.arange(MAX_NMS + 1, dtype=torch.float64)) * U16).float()
        s[-4:] = s[-1]
        img, meta = ranked_layout(n, s, range(MAX_NMS - 3, MAX_NMS + 1), 105)
    pred = torch.stack((img, img, img))
    pred[1, CUT_LIVE1:, 4] = 0
    pred[2, :, 4] = 0
    return pred, meta


MULTI_KW = dict(conf_thres=0.25, iou_thres=0.45, multi_label=True)   # max_det stays 300: 20 sites x 10 classes and the witnesses


@functools.lru_cache(maxsize=None)
def multi_cut_scene():
    """Scene 2 -> ((1, 4096, 15), meta): the tie layout over 40960 (row, class) candidates; every 512-row chunk emits more than 4096
    entries, so the emit stores them directly."""
    img, meta = tie_layout(4096, 10, 201, 20, ranks=lambda r: (0, 1, r - 2, r - 1, r, r + 1, -1), borders=list(range(SEL_CHUNK, 40960, SEL_CHUNK)))
    return img[None], meta


SELECT_CARRY_BORDER = SEL_CHUNK * SCAN_WIDTH                          # 1,048,576


@functools.lru_cache(maxsize=None)
def select_carry_scene():
    """Scene 6 -> ((1, 110000, 15), meta): 1.1 M candidates, more than 256 select chunks; the tie lies late in the image, about half of its
    r taken cells past candidate index 1,048,576."""
    g = torch.Generator().manual_seed(601)
    early = 95000 + torch.randperm(9800, generator=g)[:750]
    late = 104900 + torch.randperm(5100, generator=g)[:2250]
    img, meta = tie_layout(110000, 10, 602, 20, tie_rows=torch.cat((early, late)), ranks=lambda r: (0, r - 1, r, -1),
                           borders=[SELECT_CARRY_BORDER])
    return img[None], meta


# ------------------------------------------------------------------------------------------------ scene 3: the whole order
ORDER_SIZES = (1, 255, 256, 257, 2047, 2048, 2049, 4097, 30000)
ORDER_LATTICE = dict(box=12.0, pitch=20.0, per_row=200)


@functools.lru_cache(maxsize=None)
def order_scene(n):
    """n disjoint boxes, scores on 64 levels in [-0.25, 0.75); rows 10..13 hold +0.0, -0.0, -0.0, +0.0 -> (boxes xyxy, scores)."""
    g = torch.Generator().manual_seed(300 + n)
    boxes = site_xyxy(torch.randperm(n, generator=g), **ORDER_LATTICE)
    scores = (torch.randint(0, 64, (n,), generator=g).float() - 16) / 64
    if n >= 14:
        scores[10:14] = torch.tensor([0.0, -0.0, -0.0, 0.0])
    return boxes, scores


# ------------------------------------------------------------------------------------------------ scene 4: rounds, kept list, max_det
ROUNDS_KW = dict(conf_thres=0.25, iou_thres=0.45)
ROUNDS_MAX_DET = (511, 512, 513, 1020, 1021, 1024)


@functools.lru_cache(maxsize=None)
def rounds_scene(leaders=1100):
    """-> ((2, leaders + 1500, 7), meta).  Leaders: distinct sites, the highest scores, 4 * 2^-14 apart.  300 followers copy the box and
    class of a leader among the first 400 one 2^-14 below its score (the same round: the round's matrix and its serial resolve decide);
    1200 copy one with a score below every leader (rounds later: the kept list decides).  Image 1 is image 0 with its rows reversed; no
    two scores are equal, so it has the same output."""
    g = torch.Generator().manual_seed(400 + leaders)
    u = 2.0 ** -14
    n = leaders + 1500
    lead_score = 0.95 - 4 * u * torch.arange(leaders, dtype=torch.float64)
    near_of = torch.randperm(400, generator=g)[:300]
    far_of = torch.randint(0, 400, (1200,), generator=g)
    leader = torch.cat((torch.arange(leaders), near_of, far_of))
    score = torch.cat((lead_score, lead_score[near_of] - u, 0.3 + u * (torch.randperm(1200, generator=g).double() + 1))).float()
    lead_site = torch.randperm(leaders, generator=g)
    shuffle = torch.randperm(n, generator=g)
    leader, score = leader[shuffle], score[shuffle]
    img = torch.zeros(n, 7)
    img[:, :4] = site_xywh(lead_site[leader])
    img[:, 4] = 1.0
    img[torch.arange(n), 5 + leader % 2] = score
    rank = torch.empty(n, dtype=torch.long)
    rank[select(score, n)] = torch.arange(n)
    is_leader = shuffle < leaders
    lead_rank = torch.empty(leaders, dtype=torch.long)
    lead_rank[leader[is_leader]] = rank[is_leader]
    meta = dict(leaders=leaders, follower_drop=(rank - lead_rank[leader])[~is_leader])
    return torch.stack((img, img.flip(0))), meta


# ------------------------------------------------------------------------------------------------ scene 5: the count scan's carry
CARRY_KW = dict(conf_thres=0.25, iou_thres=0.45)
CARRY_NC = (1, 80)


def carry_chunk_rows(nc):
    return 512 if nc == 1 else 256


@functools.lru_cache(maxsize=None)
def carry_scene(nc):
    """-> ((1, n, 5 + nc), meta) with n = 257 chunks and a few rows: more count chunks than one pass of the scan covers.  About 600 rows
    are candidates (objectness = the score, one class at 1.0), in chunks 0, 255, 256, the last partial chunk and at random; twelve in
    chunks >= 256 have the highest scores and sites of their own.  The last row of chunk 255 and the first of chunk 256 tie in confidence
    on one site, the later one shifted by 1 px: the earlier one must win."""
    g = torch.Generator().manual_seed(500 + nc)
    ch = carry_chunk_rows(nc)
    tail = 37 if nc == 1 else 5
    n = 256 * ch + ch + tail

    def some(chunk, k, rows=ch):
        return chunk * ch + torch.randperm(rows, generator=g)[:k]

    pair = torch.tensor([256 * ch - 1, 256 * ch])
    late = torch.cat((some(256, 8), some(257, 4, tail)))
    rows = torch.cat((some(0, 40), some(255, 40), some(256, 40), some(257, min(tail, 20), tail), torch.randperm(n, generator=g)[:450]))
    rows = rows.unique()
    rows = rows[~torch.isin(rows, torch.cat((pair, late)))]
    k = rows.numel()
    img = torch.zeros(n, 5 + nc)
    img[:, :4] = site_xywh(torch.randint(0, 100, (n,), generator=g))
    img[:, 5] = 0.9                                                   # rows without objectness must stay out whatever their class says
    cls = torch.tensor([3 % nc, nc - 1])[torch.randint(0, 2, (n,), generator=g)]
    every = torch.cat((rows, late, pair))
    img[every, 5:] = 0
    img[every, 5 + cls[every]] = 1.0
    img[rows, 4] = (0.3 + (torch.randperm(k, generator=g).double() + 1) * 2.0 ** -11).float()
    img[late, :4] = site_xywh(100 + torch.arange(12))
    img[late, 4] = (0.9 + torch.arange(12).double() * 2.0 ** -11).float()
    img[pair, :4] = site_xywh([112, 112])
    img[pair[1], 0] += 1.0
    img[pair, 4] = 0.8
    img[pair, 5:] = 0
    img[pair, 5 + nc - 1] = 1.0
    return img[None], dict(chunk_rows=ch, late=late, pair=pair, n_cand=k + 14)


# ------------------------------------------------------------------------------------------------ expected outputs, computed once
def margins_hold(margins):
    """R.MIN_MARGIN on every threshold decision a rule recorded ('gap' compares two scores, and the scenes tie scores on purpose)."""
    return all(margins[k] >= R.MIN_MARGIN for k in ('thr', 'score', 'merge') if k in margins)


@functools.lru_cache(maxsize=None)
def cut_expected(kind, mode='iou'):
    margins = {}
    return R.non_max_suppression(cut_scene(kind)[0].clone(), nms=mode, margins=margins, **CUT_KW), margins


@functools.lru_cache(maxsize=None)
def multi_cut_expected():
    return O.non_max_suppression(multi_cut_scene()[0].clone(), **MULTI_KW)


@functools.lru_cache(maxsize=None)
def select_carry_expected():
    return O.non_max_suppression(select_carry_scene()[0].clone(), **MULTI_KW)


@functools.lru_cache(maxsize=None)
def order_expected(n):
    return torch.argsort(order_scene(n)[1], descending=True, stable=True)


@functools.lru_cache(maxsize=None)
def rounds_expected(leaders, max_det, merge=False, dtype=None):
    """-> (rows per image, margins, info)"""
    margins, info = {}, []
    pred = rounds_scene(leaders)[0].clone()
    if not merge:
        return O.non_max_suppression(pred, max_det=max_det, **ROUNDS_KW), margins, info
    return R.non_max_suppression(pred, max_det=max_det, merge=True, dtype=dtype, margins=margins, info=info, **ROUNDS_KW), margins, info


@functools.lru_cache(maxsize=None)
def carry_expected(nc):
    return O.non_max_suppression(carry_scene(nc)[0].clone(), **CARRY_KW)
