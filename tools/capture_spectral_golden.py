"""Writes tests/golden/g17_spectral.npz: the auto-dispersion loop of the reference's spectral analyser
(spectralAnalyserUI.py:271-300), restated in tests/spectral_ref.py on NumPy's own np.interp / np.corrcoef, for five
synthetic spectra whose spectral axis is the atlas sampled at a known dispersion.

    python tools/capture_spectral_golden.py [out.npz]

Each case keeps its inputs (spectrum2 uint16 [W], anchor_x, the anchor wavelength) and what the loop answers (corr [3W],
scales [3W], the arg-maximum).  Parity is with the reference, not with the truth: at W = 200 around H-alpha a true
dispersion of 0.05 A/px comes out as 0.0609."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import spectral_ref as ref          # noqa: E402

ATLAS = os.path.join(REPO, 'tests', 'golden', 'alps.npz')
H_ALPHA, NA_D2 = 6562.808, 5889.973

# name: (W, anchor wavelength, true dispersion, anchor_x)
CASES = {
    'ha200': (200, H_ALPHA, 0.05, 101.37),
    'ha600': (600, H_ALPHA, 0.05, 297.81),
    'na600': (600, NA_D2, 0.04, 310.42),
    'ha_edge': (400, H_ALPHA, 0.07, 6.63),
    'ha_right': (300, H_ALPHA, 0.03, 291.2),
}


def synth_spectrum(atlas, w, anchor_wavelength, dispersion, anchor_x, peak=52000.0, seed=0):
    """uint16 [W]: the atlas at lambda = anchor + (p - anchor_x) * dispersion, a slow continuum tilt, a little noise."""
    a = ref.atlas_axis(atlas['first'], atlas['last'], atlas['step'])
    p = np.arange(w, dtype=np.float64)
    lam = anchor_wavelength + (p - anchor_x) * dispersion
    prof = np.interp(lam, a, atlas['y'] / 255)
    tilt = 1.0 + 0.1 * (p / w - 0.5)
    noise = np.random.default_rng(seed).normal(0.0, 0.004, w)
    return np.clip(np.rint(peak * (prof * tilt + noise)), 1, 65535).astype(np.uint16)


def main(out=os.path.join(REPO, 'tests', 'golden', 'g17_spectral.npz')):
    atlas = dict(np.load(ATLAS))
    blob = {}
    for name, (w, lam, disp, ax) in CASES.items():
        s2 = synth_spectrum(atlas, w, lam, disp, ax)
        corr, scales = ref.correlations(s2, ax, lam, atlas['first'], atlas['last'], atlas['step'], atlas['y'])
        i = int(np.argmax(corr))
        top2 = np.sort(corr)[-2:]
        print('%-9s W=%4d true %.4f -> %.6f (index %d, top-two gap %.2e)' % (name, w, disp, scales[i], i, top2[1] - top2[0]))
        blob.update({name + '_spectrum2': s2, name + '_anchor_x': np.float64(ax), name + '_anchor_wavelength': np.float64(lam),
                     name + '_true_dispersion': np.float64(disp), name + '_corr': corr, name + '_scales': scales,
                     name + '_index': np.int64(i)})
    blob['cases'] = np.array(list(CASES))
    np.savez_compressed(out, **blob)
    print('wrote', out)


if __name__ == '__main__':
    main(*sys.argv[1:])
