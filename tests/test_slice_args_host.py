"""The channel-slice rule of the C ABI, at every entry point that takes a slice (include/somi_hip.h, Conventions; slice_fault() in csrc/common.h).

One table, one row per entry point: a valid argument tuple at the smallest legal shape and its slices.  Every slice is broken in six ways, one at
a time; each must come back as SOMI_EINVAL with a message that names the slice's pointer parameter as the header spells it, and the valid tuple
must NOT come back as SOMI_EINVAL (a rule that is too strict shows up here, without a GPU).

Pointers are made-up aligned integers: nothing is allocated and nothing is dereferenced, so a call that passed the check would launch a kernel on
a made-up address.  The table therefore runs in a child process that has no device (HIP_VISIBLE_DEVICES=-1), and the child verifies
torch.cuda.device_count() == 0 BEFORE its first call into the library; with a device visible it calls nothing and the tests skip.  Without a
device an accepted call returns the launch failure (a positive hipError_t)."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'somi_hip.h')
EINVAL = -1
BIG = 1 << 40                     # a workspace size no plan exceeds


class Sl:
    """A slice argument: the names of its pointer, stride and offset parameters as the header spells them ('d.' = a field of the somi_conv_desc the
    entry point takes), and the width its kernels touch at the row's shape.  The valid tuple holds it as [4, 4 + width) of width + 8 channels.
    shared: stride and offset are another slice's too (that slice comes first and is the one named), so only the pointer is broken here."""

    def __init__(self, ptr, cs, coff, width, optional=False, shared=False):
        self.ptr, self.cs, self.coff, self.width, self.optional, self.shared = ptr, cs, coff, width, optional, shared

    def mutations(self):
        cs, coff = self.width + 8, 4
        m = [('pointer + 4 bytes', {self.ptr: '+4'}), ('pointer NULL', {self.ptr: None})]
        if not self.shared:
            m += [('coff = -4', {self.coff: -4}), ('coff + width = cs + 4', {self.coff: cs + 4 - self.width}), ('coff + 2', {self.coff: coff + 2}),
                  ('cs + 2', {self.cs: cs + 2})]
        return m


def x_like(*names, width=8, **kw):
    """Slices that follow the header's usual spelling: pointer `n`, stride `n_cs`, offset `n_coff`."""
    return [Sl(n, n + '_cs', n + '_coff', width, **kw) for n in names]


CONV = {'d.w': 0, 'd.B': 1, 'd.H': 2, 'd.W': 2, 'd.Cin': 8, 'd.Ho': 2, 'd.Wo': 2, 'd.Cout': 8, 'd.kh': 1, 'd.kw': 1, 'd.stride': 1, 'd.pad': 0, 'd.dil': 1}
RES2 = Sl('d.residual2', 'd.res2_cs', 'd.res2_coff', 8, optional=True)
IMG = {'B': 1, 'H': 2, 'W': 2, 'C': 8}
PIX = {'B': 1, 'HW': 4, 'C': 8}
NPIX = {'npix': 4, 'C': 8}
BN = dict(NPIX, act=1, order=0)
GC = {'B': 1, 'H': 2, 'W': 2, 'C1': 8, 'C2': 8, 'groups': 1, 'k': 1, 'stride': 1}
POOL2 = dict(IMG, stride=2, pad_l=0, pad_r=0, pad_t=0, pad_b=0)
SPP = dict(IMG, nk=3, k0=5, k1=9, k2=13)

# row (entry point, or 'entry point/variant') -> (scalar arguments of the valid tuple, slices, pointer parameters the valid tuple leaves NULL).  Every other pointer parameter gets
# a made-up 16-byte aligned address, every other scalar 0.
TABLE = {
    'somi_conv2d_nhwc_f32': (dict(CONV), [Sl('d.x', 'd.x_cs', 'd.x_coff', 8), Sl('d.y', 'd.y_cs', 'd.y_coff', 8),
                                          Sl('d.residual', 'd.res_cs', 'd.res_coff', 8, optional=True), RES2], ()),
    'somi_conv2d_dgrad_nhwc_f32': (dict(CONV), x_like('dy', 'dx') + [Sl('accumulate', 'acc_cs', 'acc_coff', 8, optional=True), RES2], ()),
    'somi_conv2d_wgrad_nhwc_f32': (dict(CONV, workspace_bytes=BIG), x_like('x', 'dy'), ()),
    'somi_gconv2d_nhwc_f32': (dict(GC, w_cs=8, Cw=8), x_like('x', 'y') + [Sl('residual', 'res_cs', 'res_coff', 8, optional=True)], ()),
    'somi_gconv2d_dgrad_nhwc_f32': (dict(GC, w_cs=8, Ho=2, Wo=2, Cx=8), x_like('dy', 'dx') + x_like('acc1', 'acc2', optional=True), ()),
    'somi_gconv2d_wgrad_nhwc_f32': (dict(GC, Ho=2, Wo=2, workspace_floats=BIG), x_like('x', 'dy'), ()),
    'somi_psa_attention_f32': ({'B': 1, 'N': 4, 'heads': 1}, x_like('qkv', width=128) + x_like('o', width=64), ()),
    'somi_psa_attention_backward_f32': ({'B': 1, 'N': 4, 'heads': 1}, x_like('qkv', width=128) + x_like('o', width=64) +
                                        [Sl('dout', 'do_cs', 'do_coff', 64), Sl('dqkv', 'g_cs', 'g_coff', 128)], ()),
    'somi_carafe_nhwc_f32': (dict(IMG, k_up=3), x_like('x') + [Sl('logits', 'l_cs', 'l_coff', 36), Sl('out', 'o_cs', 'o_coff', 8)], ()),
    'somi_carafe_bwd_nhwc_f32': (dict(IMG, k_up=3), [Sl('dout', 'd_cs', 'd_coff', 8)] + x_like('x', 'dx') + [Sl('dlogits', 'dl_cs', 'dl_coff', 36)], ()),
    'somi_dysample_nhwc_f32': (dict(IMG, groups=1), x_like('x') + [Sl('offset', 'f_cs', 'f_coff', 8), Sl('out', 'o_cs', 'o_coff', 8)], ()),
    'somi_dysample_bwd_nhwc_f32': (dict(IMG, groups=1), [Sl('dout', 'd_cs', 'd_coff', 8)] + x_like('x') + [Sl('offset', 'f_cs', 'f_coff', 8)] +
                                   x_like('dx') + [Sl('doffset', 'df_cs', 'df_coff', 8)], ()),
    'somi_maxpool2_nhwc_f32': (dict(POOL2), x_like('x', 'y'), ()),
    'somi_maxpool2_bwd_nhwc_f32': (dict(POOL2), x_like('dy', 'dx'), ()),
    'somi_spp_pool_nhwc_f32': (dict(SPP), [Sl('buf', 'cs', 'x_coff', 32)], ()),
    'somi_spp_pool_bwd_nhwc_f32': (dict(SPP), [Sl('dbuf', 'cs', 'x_coff', 32)], ()),
    'somi_sppf_pool_nhwc_f32': (dict(IMG), [Sl('buf', 'cs', 'x_coff', 32)], ()),
    'somi_sppf_pool_codes_nhwc_f32': (dict(IMG), [Sl('buf', 'cs', 'x_coff', 32)], ()),
    'somi_sppf_pool_bwd_nhwc_f32': (dict(IMG), [Sl('dbuf', 'cs', 'x_coff', 32), Sl('buf', 'cs', 'x_coff', 32, optional=True, shared=True)], ()),
    'somi_global_pool_nhwc_f32': (dict(PIX), x_like('x'), ()),
    'somi_global_pool_act_nhwc_f32': (dict(PIX, act=1), x_like('x'), ()),
    'somi_affine_silu_pool_nhwc_f32': (dict(PIX), x_like('x', 'z'), ()),
    'somi_chan_stats_nhwc_f32': (dict(PIX), x_like('x'), ()),
    'somi_cbam_apply_nhwc_f32': (dict(IMG, k=3), x_like('x', 'y'), ()),
    'somi_bn_stats_nhwc_f32': (dict(NPIX), x_like('x'), ()),
    'somi_bn_stats_act_nhwc_f32': (dict(NPIX, act=1), x_like('x'), ()),
    'somi_bn_local_sums_f64': (dict(NPIX), x_like('x'), ('part_sum', 'part_sumsq')),       # x is read (and checked) only without partial rows
    'somi_bn_act_backward_sums_f64': (dict(BN), x_like('dz', 'x'), ()),
    'somi_bn_act_backward_apply_sync_f32': (dict(BN, nranks=1), x_like('dz', 'x', 'dx'), ()),
    'somi_chan_affine_act_nhwc_f32': (dict(BN), x_like('x', 'z') + [Sl('residual', 'res_cs', 'res_coff', 8, optional=True)], ()),
    'somi_bn_act_backward_nhwc_f32': (dict(BN, batch_stats=1), x_like('dz', 'x', 'dx'), ()),
    'somi_bn_act_backward_pooled_nhwc_f32': (dict(PIX, act=1, order=0), x_like('dz', optional=True) + x_like('x', 'dx'), ()),
    'somi_add_nhwc_f32': (dict(NPIX), x_like('a', 'b') + [Sl('out', 'o_cs', 'o_coff', 8)], ()),
    'somi_chan_sum_nhwc_f32': (dict(NPIX), x_like('x'), ()),
    'somi_cbam_bn_bwd_reduce_f32': (dict(PIX), x_like('d', 'y'), ()),
    'somi_cbam_bn_bwd_apply_f32': (dict(PIX), x_like('d', 'y', 'dx'), ()),
    'somi_cbam_bwd_pixel_argmax_f32': (dict(PIX), [Sl('dt2', 'd_cs', 'd_coff', 8)] + x_like('t'), ()),
    'somi_cbam_bwd_chan_f32': (dict(PIX), [Sl('dt2_inout', 'd_cs', 'd_coff', 8)] + x_like('t'), ()),
    'somi_pool_bwd_add_nhwc_f32': (dict(PIX), [Sl('dt_inout', 'd_cs', 'd_coff', 8)], ()),
    'somi_resample_slice_nhwc_f32': ({'B': 1, 'Hs': 2, 'Ws': 2, 'C': 8, 'up': 1}, x_like('src', 'dst'), ()),
    'somi_space_to_depth_nhwc_f32': ({'B': 1, 'Ho': 2, 'Wo': 2, 'C': 8}, x_like('x') + x_like('y', width=32), ()),
    'somi_space_to_depth_nhwc_f32/inverse': ({'B': 1, 'Ho': 2, 'Wo': 2, 'C': 8, 'inverse': 1}, x_like('x', width=32) + x_like('y'), ()),   # widths swap
}


def entry(row):
    """The entry point of a row: a second row of one entry point (a branch with other widths) is keyed 'name/variant'."""
    return row.split('/')[0]


def prototypes():
    """name -> [(parameter name, 'desc' | 'stream' | 'ptr' | 'num')] of every `int somi_*(...)` the header declares."""
    def kind(p):
        return 'desc' if 'somi_conv_desc' in p else 'stream' if 'somi_stream_t' in p else 'ptr' if '*' in p else 'num'
    text = re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r'\bint\s+(somi_\w+)\s*\(([^;{]*?)\)\s*;', text):
        out[name] = [(re.findall(r'\w+', p)[-1], kind(p)) for p in params.split(',') if p.strip() != 'void']
    return out


# ---------------------------------------------------------------------------------------------------------------- the child: no device, or no call
def _call(L, _lib, params, values):
    """One call.  values: parameter name (or 'd.field') -> int, None (NULL) or '+4' (the made-up address plus 4 bytes)."""
    import ctypes
    addr = {}

    def pointer(name):
        addr.setdefault(name, 0x10000 + 0x1000 * len(addr))
        v = values.get(name, 0)
        return None if v is None else addr[name] + (4 if v == '+4' else 0)

    desc = _lib.ConvDesc()
    for field, ctype in _lib.ConvDesc._fields_:
        key = 'd.' + field
        if ctype is ctypes.c_void_p:
            setattr(desc, field, pointer(key) if key in values else None)
        else:
            setattr(desc, field, values.get(key, 0))
    args = []
    for name, kind in params:
        if kind == 'desc':
            args.append(ctypes.byref(desc))
        elif kind == 'stream':
            args.append(None)
        else:
            args.append(pointer(name) if kind == 'ptr' else values.get(name, 0.1 if name in ('eps', 'momentum') else 0))
    rc = getattr(L, values['fn'])(*args)
    return rc, L.somi_last_error().decode(errors='replace')


def _child():
    import torch
    n = torch.cuda.device_count()
    if n != 0:                                               # the guard: with a device visible nothing is called
        print(json.dumps({'devices': n}))
        return
    sys.path.insert(0, os.path.join(ROOT, 'yolo-somi_amd'))
    from somi_amd import _lib
    L = _lib.lib()
    protos = prototypes()
    results = {}
    for row, (scalars, slices, null) in TABLE.items():
        valid = dict(scalars, fn=entry(row), **{p: None for p in null})
        for s in slices:
            valid.update({s.ptr: 0, s.cs: s.width + 8, s.coff: 4})
        cases = [('valid', None, valid)]
        for s in slices:
            cases += [(what, s, dict(valid, **change)) for what, change in s.mutations()]
        results[row] = [{'case': what, 'slice': s.ptr.split('.')[-1] if s else None, 'optional': bool(s and s.optional)} |
                        dict(zip(('rc', 'error'), _call(L, _lib, protos[entry(row)], values))) for what, s, values in cases]
    print(json.dumps({'devices': 0, 'results': results}))


# ---------------------------------------------------------------------------------------------------------------- the tests
_cache = {}


def child_results():
    if 'run' not in _cache:                                  # one child for the whole table, also when it fails
        env = dict(os.environ, HIP_VISIBLE_DEVICES='-1')
        _cache['run'] = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    r = _cache['run']
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    if out['devices'] != 0:
        pytest.skip(f"{out['devices']} GPU(s) visible to the child despite HIP_VISIBLE_DEVICES=-1: made-up addresses are never handed to a process "
                    "that could launch on them")
    return out['results']


@pytest.mark.parametrize('fn', sorted(TABLE))
def test_entry_point_checks_every_slice(fn):
    cases = child_results()[fn]
    slices = TABLE[fn][1]
    assert len(cases) == 1 + sum(len(s.mutations()) for s in slices)
    for c in cases:
        what = f"{fn}: {c['slice']}: {c['case']}: returned {c['rc']}, \"{c['error']}\""
        if c['case'] == 'valid' or (c['case'] == 'pointer NULL' and c['optional']):
            assert c['rc'] != EINVAL, what + ' - a valid tuple is refused'
            assert c['rc'] > 0, what + ' - without a device an accepted call ends in the launch failure'
        else:
            assert c['rc'] == EINVAL, what + ' - a bad slice is let through'
            assert re.search(r'\b%s = \[' % re.escape(c['slice']), c['error']), what + ' - the message does not name the slice'


def test_every_slice_taking_entry_point_has_a_row():
    """A new entry point with a `_coff` parameter fails here until it has a row (somi_conv2d_nhwc_f32 takes its slices in the descriptor)."""
    takes = {name for name, params in prototypes().items() if any(p.endswith('_coff') for p, _ in params)} | {'somi_conv2d_nhwc_f32'}
    assert len(takes) >= 40
    rows = {entry(row) for row in TABLE}
    assert takes == rows, f'no row: {sorted(takes - rows)}; no such entry point: {sorted(rows - takes)}'


def test_rows_name_parameters_the_header_declares():
    """A misspelt name in a row would silently become a scalar 0 / an untouched argument."""
    from somi_amd import _lib
    fields = {'d.' + f for f, _ in _lib.ConvDesc._fields_}
    for fn, (scalars, slices, null) in TABLE.items():
        names = {p for p, _ in prototypes()[entry(fn)]} | fields
        used = set(scalars) | set(null) | {n for s in slices for n in (s.ptr, s.cs, s.coff)}
        assert used <= names, (fn, sorted(used - names))


if __name__ == '__main__':
    _child()
