"""The atlas fixtures the spectral analyser's tests and the line maps' --atlas tests share: the atlas itself (atlas_npz) and a
synthetic scan whose spectral axis is the atlas at a known dispersion (atlas_scan)."""
import os

import numpy as np
import pytest

from tests import spectral_ref as ref
from tests.linemaps_util import write_scan

ATLAS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'alps.npz')
H_ALPHA = 6562.808
IH, IW, N = 720, 640, 96                    # the atlas scan
TRUE_DISPERSION = 0.04


@pytest.fixture(scope='module')
def atlas_npz():
    z = dict(np.load(ATLAS))
    z['a'] = ref.atlas_axis(z['first'], z['last'], z['step'])
    z['yv'] = z['y'] / 255
    return z


def core_wavelength(atlas_npz):
    """The atlas's own H-alpha core (its darkest point within 1 A of 6562.808): the line fit finds that, so the scan puts it
    on the curve and the analyser is anchored on it."""
    near = np.flatnonzero(np.abs(atlas_npz['a'] - H_ALPHA) <= 1.0)
    return float(atlas_npz['a'][near[np.argmin(atlas_npz['y'][near])]])


@pytest.fixture(scope='module')
def atlas_scan(atlas_npz, tmp_path_factory):
    """[N, IH, IW] uint16 (file layout, no rotation): a limb-darkened disk crossing the slit, every slit row the atlas at
    TRUE_DISPERSION around H-alpha with the line centre on a curve."""
    y = np.arange(IH, dtype=np.float64)
    x = np.arange(IW, dtype=np.float64)
    yc = y - IH / 2.0
    centre = IW / 2.0 + 4e-5 * yc * yc + 0.004 * yc
    lam = core_wavelength(atlas_npz) + (x[None, :] - centre[:, None]) * TRUE_DISPERSION
    prof = np.interp(lam, atlas_npz['a'], atlas_npz['yv'])
    lit = ((y > 0.06 * IH) & (y < 0.94 * IH)).astype(np.float64)
    frames = np.empty((N, IH, IW), dtype=np.uint16)
    for k in range(N):
        r2 = ((k - N / 2.0) / (0.42 * N)) ** 2 + (yc / (0.44 * IH)) ** 2
        bright = np.where(r2 < 1.0, 0.35 + 0.65 * np.sqrt(np.clip(1.0 - r2, 0.0, 1.0)), 0.02) * lit
        noise = np.random.default_rng([7, k]).standard_normal((IH, IW))
        frames[k] = np.clip(np.rint((0.8 * bright[:, None] * prof + 0.003 * noise) * 65535.0), 0, 65535)
    return write_scan(tmp_path_factory, 'atlas_scan', frames)
