"""NumPy restatement of the reference's spectral analyser, numeric half (spectralAnalyserUI.py), written for the tests:
the auto-dispersion loop (:271-300) on the real np.interp / np.corrcoef, and the wavelength -> pixel shift step (:184-210,
:240-260).  The GUI around it is not restated."""
import numpy as np

EXCLUDE = 5          # the exclusion half-width around the anchor line (:285)


def atlas_axis(first, last, step):
    """np.arange(first, last, step) as the reference builds it (:61)."""
    return np.arange(first, last, step)


def select_run(x, lo, hi):
    """[k0, k1] of the contiguous run with lo <= x < hi (select, :41-48); ValueError when empty, as min() of nothing raises."""
    v = np.where(np.logical_and(lo <= x, x < hi))[0]
    return int(min(v)), int(max(v))


def window(anchor_x, w):
    """The slice the reference overwrites with the mean (:284-287): note the W - 1 bound."""
    return slice(max(0, int(anchor_x) - EXCLUDE), min(int(anchor_x) + EXCLUDE, w - 1))


def log_spectrum(spectrum2, anchor_x):
    """np.log of the uint16 spectrum (float32), the window set to its float32 mean (:286-287)."""
    lspec = np.log(spectrum2)
    lspec[window(anchor_x, spectrum2.shape[0])] = np.mean(lspec)
    return lspec


def interp_row(a, yv, anchor_wavelength, anchor_x, scale, w):
    """The atlas scaled by one guess, interpolated onto the W pixels, its window set to its mean (:277-285)."""
    x = (a - anchor_wavelength) / scale + anchor_x
    k0, k1 = select_run(x, 0, w)
    u = np.interp(np.arange(w), x[k0:k1 + 1], yv[k0:k1 + 1])
    u[window(anchor_x, w)] = np.mean(u)
    return u


def scale_guesses(w):
    return np.linspace(0.02, 0.12, w * 3)


def correlations(spectrum2, anchor_x, anchor_wavelength, first, last, step, y, scales=None):
    """-> (corr [3W], scales [3W]) of the auto-dispersion loop."""
    w = spectrum2.shape[0]
    a = atlas_axis(first, last, step)
    yv = y / 255
    scales = scale_guesses(w) if scales is None else scales
    lspec = log_spectrum(spectrum2, anchor_x)
    corr = np.array([np.corrcoef(interp_row(a, yv, anchor_wavelength, anchor_x, s, w), lspec)[0, 1] for s in scales])
    return corr, scales


def auto_dispersion(spectrum2, anchor_x, anchor_wavelength, atlas):
    """-> (dispersion, corr, scales); atlas = dict(first, last, step, y) in alps.npz's layout."""
    corr, scales = correlations(spectrum2, anchor_x, anchor_wavelength, atlas['first'], atlas['last'], atlas['step'], atlas['y'])
    return scales[np.argmax(corr)], corr, scales


def shift_for_wavelength(wavelength, anchor_wavelength, dispersion, fit, iw):
    """-> (shift, within [ih] bool) of :245-250; the caller decides error / warning from `within`."""
    shift = int((wavelength - anchor_wavelength) / dispersion)
    positions = shift + fit[:, 3]
    within = np.logical_and(0 <= positions, positions <= iw)
    return shift, within
