"""What tests/test_contrast_cases_cpu.py and tests/test_contrast_oracle_gpu.py share: the per-call knobs of a case, the library's
plan for it (shg_contrast_plan_query: no GPU needed), and the oracle's transversalium for the cases that have one."""
import ctypes

import numpy as np

from oracle import shg_oracle as orc
from tests import contrast_cases as cc

FIELDS = ('batched', 'disks', 'route', 'bits', 'clip', 'slice_rows', 'slices', 'chunk_rows', 'rank0', 'rank1', 'from_top', 'blend_px',
          'blend_tiled', 'lut_all', 'window', 'fused')


def set_knobs(monkeypatch, env):
    """The six per-call knobs as the case wants them: those it does not name are unset."""
    for name in cc.KNOBS:
        if name in env:
            monkeypatch.setenv(name, env[name])
        else:
            monkeypatch.delenv(name, raising=False)


def asks_fused(c):
    """Whether the stage is asked in a way that lets the histogram kernel form the images (it does so only where it batches)."""
    return not (c['keep'] and c['trans']) and c['env'].get('SHG_FUSE_SCALE') != '0'


def plan_of(c):
    """The plan of the case's contrast stage under the knobs now in the environment, by name."""
    from solex_ser_recon_en_amd import _lib
    out = (ctypes.c_int64 * 16)()
    h, w = c['shape'][0], c['out_w']
    pitch = cc.pitch_of(w)
    err = _lib.lib.shg_contrast_plan_query(c['k'], h, w, pitch, pitch, 0, c['clip_limit'], c['tiles'], int(asks_fused(c)), 1, -1, out)
    assert err == 0, _lib.last_error()
    p = dict(zip(FIELDS, out))
    p['route'] = cc.ROUTES[p['route']]
    return p


def check_plan(c, p):
    """The plan against what the case's id promises."""
    _, _, th, tw = cc.grid(c['shape'][0], c['out_w'], c['tiles'])
    assert p['clip'] == (c['clip'] or 0), (c['id'], p)
    for name, want in c['expect'].items():
        if name == 'several_slices':
            assert p['slices'] > 1, (c['id'], p)
        elif name == 'several_chunks':
            assert p['slice_rows'] > p['chunk_rows'] and th > p['chunk_rows'], (c['id'], p)
        elif name == 'big':
            assert p['slice_rows'] == (65535 if want else 32768) // tw, (c['id'], p)
        elif name == 'ktop':
            assert (p['rank0'], p['rank1']) == (want, want - 1), (c['id'], p)
        else:
            assert p[name] == want, (c['id'], name, p)
    if p['from_top']:
        assert (p['rank0'], p['rank1']) == cc.k_tops(c['shape'][0] * c['out_w']) and p['rank0'] <= p['clip'], (c['id'], p)


def oracle_transversalium(img):
    """-> (the oracle's corrected image, its row factors) with the circle, borders and window the cases use."""
    h, w = img.shape
    circle, borders, window = cc.transversalium_of(h, w)
    return orc.correct_transversalium2(img, circle, borders, window)
