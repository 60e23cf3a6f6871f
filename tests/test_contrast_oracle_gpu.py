"""The batched contrast stage (shg_stage_process_frames: csrc/stages.hip, csrc/clahe.hip, csrc/post.hip) against the oracle, bit for
bit, on every route of its plan.  The cases and what each is there for: tests/contrast_cases.py (checked without a GPU by
tests/test_contrast_cases_cpu.py, which also holds every case to the route its id names); the reference: tests/contrast_ref.py,
the oracle's own functions composed.  No tolerance anywhere: the path is integer arithmetic, or float32 restated operation by
operation.  A transversalium's row factors come from float64 host mathematics held to the oracle by their own tests; here the
factors the stage returns go into the reference as data, and the image they give is compared with the oracle's own through
conftest.flips."""
import ctypes

import numpy as np
import pytest

from tests import contrast_cases as cc
from tests import contrast_ref as ref
from tests import contrast_util as cu
from tests.conftest import flips

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def stages():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from solex_ser_recon_en_amd import stages as _stages
    return _stages


def upload(frames):
    """The disks as views into a pitched store, as production's are."""
    k, (h, w) = len(frames), frames[0].shape
    store = torch.zeros((k, h, cc.pitch_of(w)), dtype=torch.uint16, device='cuda')
    for i, img in enumerate(frames):
        store[i, :, :w] = torch.from_numpy(np.ascontiguousarray(img).view(np.int16)).cuda().view(torch.uint16)
    return [store[i, :, :w] for i in range(k)]


def download(t):
    return np.asarray(t.cpu().view(torch.int16).numpy()).view(np.uint16).copy()


def transversalium_for(h, w):
    from solex_ser_recon_en_amd import solex_util
    circle, borders, window = cc.transversalium_of(h, w)
    return dict(circle=circle, borders=borders, taps=solex_util.savgol_taps(window), window=window)


def reselected():
    """How many disks the stage selected their frame percentile over the image for, since shg_host_timing_enable(1)."""
    from solex_ser_recon_en_amd import _lib
    buf = ctypes.create_string_buffer(1 << 14)
    _lib.lib.shg_host_timing_report(buf, len(buf))
    return sum(int(line.rsplit(' ', 1)[1]) for line in buf.value.decode().splitlines() if line.startswith('frame percentile selected'))


def run_stage(stages, views, c, h, w):
    from solex_ser_recon_en_amd import _lib
    _lib.lib.shg_host_timing_enable(1)
    try:
        res = stages.process_frames(views, transversalium_for(h, w) if c['trans'] else None, c['crop'], c['disc'], c['clip_limit'], c['tiles'],
                                    keep_detrans=c['keep'])
        torch.cuda.synchronize()
        return res, reselected()
    finally:
        _lib.lib.shg_host_timing_enable(0)


def compare(label, res, i, want):
    for name in ref.PRODUCTS:
        got = download(res[name][i])
        assert got.shape == want[name].shape, (label, name, got.shape)
        np.testing.assert_array_equal(got, want[name], err_msg='%s %s[%d]' % (label, name, i))


@pytest.mark.parametrize('c', cc.CASES, ids=cc.IDS)
def test_contrast_stage_equals_the_oracle(c, stages, monkeypatch):
    """final, cl1, hc, protus and cc (and the de-transversaliumed frame where kept) of every disk equal the composed oracle's; the
    plan is the one the case names; the fall-back select ran as often as the case claims; a case made to fail fails on both sides."""
    cu.set_knobs(monkeypatch, c['env'])
    cu.check_plan(c, cu.plan_of(c))
    (h, w), frames = c['shape'], cc.frames_of(c)
    views = upload(frames)
    kw = dict(crop=c['crop'], disc=c['disc'], clip_limit=c['clip_limit'], tiles=c['tiles'])
    if c['fails']:
        bad = [ref.raises(img, **kw) for img in frames]
        assert any(bad)
        # SHG_E_ASSERT, which the binding raises as the reference's own exception type (_lib._host_error)
        with pytest.raises(AssertionError, match='rescale_brightness'):
            run_stage(stages, views, c, h, w)
        from solex_ser_recon_en_amd import _lib
        assert _lib.last_error().startswith('rescale_brightness')
        return
    res, fell_back = run_stage(stages, views, c, h, w)
    assert (res['factors'] is not None) == c['trans'] and (res['detrans'] is not None) == (c['keep'] and c['trans'])
    for i, img in enumerate(frames):
        factors = res['factors'][i] if c['trans'] else None
        want = ref.stage_reference(img, factors, **kw)
        compare(c['id'], res, i, want)
        if c['trans']:
            if res['detrans'] is not None:
                np.testing.assert_array_equal(download(res['detrans'][i]), want['detrans'], err_msg='%s detrans[%d]' % (c['id'], i))
            flips('%s detrans[%d] from the stage\'s factors' % (c['id'], i), want['detrans'], cu.oracle_transversalium(img)[0], observed=0)
    if c['fallback'] is not None:
        assert fell_back == c['fallback'], (c['id'], fell_back)


@pytest.mark.parametrize('window', ['1', None], ids=['window-forced', 'window-default'])
def test_a_series_through_one_workspace_equals_the_oracle_call_by_call(window, stages, series_references, monkeypatch):
    """The percentile window's state is carried in the stage's workspace from one call to the next: the same image twice (a hit), a
    much brighter and a much darker one (misses), back, a stack of four with mixed levels, back.  Every call equals the oracle, with
    the window forced on for single disks too (SHG_SELECT_WINDOW=1) and as the stage decides itself (from four disks)."""
    cu.set_knobs(monkeypatch, {'SHG_SELECT_WINDOW': window} if window else {})
    h, w = cc.SERIES_SHAPE
    c = dict(trans=False, crop=None, disc=cc.discs(h, w)['inside'], clip_limit=cc.clip_limit_for(cc.SERIES_CLIP, (h // 2) * (w // 2)), tiles=2, keep=False)
    for step, wants in enumerate(series_references):
        res, _ = run_stage(stages, upload(cc.series_frames(step)), c, h, w)
        for i, want in enumerate(wants):
            compare('call %d' % step, res, i, want)


@pytest.fixture(scope='module')
def series_references():
    h, w = cc.SERIES_SHAPE
    kw = dict(disc=cc.discs(h, w)['inside'], clip_limit=cc.clip_limit_for(cc.SERIES_CLIP, (h // 2) * (w // 2)), tiles=2)
    cache = {}
    out = []
    for step in range(len(cc.SERIES)):
        wants = []
        for img in cc.series_frames(step):
            key = img.tobytes()
            if key not in cache:
                cache[key] = ref.stage_reference(img, **kw)
            wants.append(cache[key])
        out.append(wants)
    return out
