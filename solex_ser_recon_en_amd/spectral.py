"""The numeric half of the reference's spectral analyser (spectralAnalyserUI.py), without its GUI: the atlas-correlation
dispersion fit (:271-300) on the GPU, and the wavelength -> pixel shift step (:184-210, :240-260) that tells a user which
`-w` shift puts a given line (He D3, Fe I, the Ca H core, ...) in the products.

    python -m solex_ser_recon_en_amd.spectral FILE --atlas alps.npz --anchor 6562.808 --goto 6559.58 [--goto ...]
        [--lines anchor_candidates.txt] [--dispersion D] [--process [SHG flags]]

prints one JSON line: anchor_x, dispersion, dispersion_rounded and, per target, its wavelength, shift and whether it is only
partially within the frame.  --process then runs the scan as `SHG_MAIN [SHG flags] -w <shifts> FILE` does.  The atlas
(alps.npz layout: first, last, step, y uint8) and the line lists (`"wavelength name"` per line) are the user's data: the
package ships neither.

Two deliberate deviations from the reference, both raising ValueError where it goes wrong quietly or obscurely:
  - a zero in the spectrum makes the reference's log -inf, every correlation NaN and the dispersion silently 0.02;
  - an anchor wavelength outside the atlas, or a guess whose atlas run inside [0, W) is empty, makes the reference fail on
    min() of an empty array.
The CLI is single-process: under torchrun (WORLD_SIZE > 1) it refuses to run.
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

from . import ops

EXCLUDE = 5                       # the exclusion half-width around the anchor line (:285)
SCALE_RANGE = (0.02, 0.12)        # the dispersion guesses, Angstrom per pixel (:274)


class Atlas:
    """A solar atlas in alps.npz's layout, its uint8 intensities uploaded once per device."""

    def __init__(self, first, last, step, y):
        self.first, self.last, self.step = first, last, step
        self.y = np.ascontiguousarray(y, dtype=np.uint8)
        # np.arange(first, last, step) (:61) is first + k * d with this d, exactly: the kernel rebuilds it from k
        self.d = float((first + step) - first)
        n = len(np.arange(first, last, step))
        if n != self.y.shape[0]:
            raise ValueError('atlas: arange(%r, %r, %r) has %d points, y has %d' % (first, last, step, n, self.y.shape[0]))
        self.n = n
        self.a_last = float(first + (n - 1) * self.d)
        self._dev = {}

    def on(self, device):
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self.y).to(device)
        return self._dev[device]


_atlases = {}


def load_atlas(path):
    """Atlas of an alps.npz-layout file (first, last, step, y uint8), cached by path."""
    key = os.path.abspath(path)
    if key not in _atlases:
        with np.load(path) as z:
            _atlases[key] = Atlas(z['first'][()], z['last'][()], z['step'][()], z['y'])
    return _atlases[key]


def load_lines(path):
    """A line list in the reference's format (`"6562.808 H(α)"` per line, load_lines :50-58) -> (wavelengths, names, labels),
    labels being name + '(' + wavelength + ')'.  The reference keeps each name's line ending; here it is dropped, and blank
    lines are skipped."""
    wavelengths, names = [], []
    with open(path, encoding='utf-8') as f:
        for line in f:
            line = line.rstrip('\r\n')
            if not line.strip():
                continue
            v = line.split(' ')
            wavelengths.append(float(v[0]))
            names.append(v[1])
    labels = [names[i] + '(' + str(wavelengths[i]) + ')' for i in range(len(names))]
    return wavelengths, names, labels


def analyse(file_or_reader, options=None):
    """Pass A and the line fit of one scan, with the options the analyser runs them under (:68-73) ->
    dict(spectrum2 = the mean image's middle row (uint16 [iw]), anchor_x = fit[ih // 2, 3], fit [ih, 4], iw, ih)."""
    from . import SHG_MAIN
    from .fits_io import make_header
    from .solex_util import compute_mean_return_fit
    from .video_reader import video_reader
    opts = SHG_MAIN.default_options() if options is None else dict(options)
    opts.update(clahe_only=True, save_fit=False, flag_display=False, _nolog=True, shift=[0], basefich0='')
    rdr = file_or_reader if hasattr(file_or_reader, 'device_stack') else video_reader(file_or_reader)
    ih, iw = int(rdr.ih), int(rdr.iw)
    mean, fit, _, _ = compute_mean_return_fit(rdr, opts, make_header(rdr), iw, ih, '')
    row = mean.t[ih // 2]
    spectrum2 = row.view(torch.int16).cpu().numpy().view(np.uint16)
    return {'spectrum2': spectrum2, 'anchor_x': float(fit[ih // 2, 3]), 'fit': fit, 'iw': iw, 'ih': ih}


def window(anchor_x, w):
    """[lo, hi) of the pixels the reference overwrites with the mean (:284-287), Python's slice rules applied (note its W - 1)."""
    lo, hi, _ = slice(max(0, int(anchor_x) - EXCLUDE), min(int(anchor_x) + EXCLUDE, w - 1)).indices(w)
    return lo, max(lo, hi)


def log_spectrum(spectrum2, anchor_x):
    """float32 np.log(spectrum2) with its window set to its float32 mean (:286-287).  ValueError on a zero pixel (the reference
    goes on with -inf and settles on the first guess)."""
    spectrum2 = np.asarray(spectrum2)
    zeros = np.flatnonzero(spectrum2 == 0)
    if zeros.size:
        raise ValueError('spectrum pixel %d is 0: its log is -inf and no correlation would be defined' % zeros[0])
    lspec = np.log(spectrum2)
    lo, hi = window(anchor_x, spectrum2.shape[0])
    lspec[lo:hi] = np.mean(lspec)
    return lspec


def scale_guesses(w, n_guesses=None):
    return np.linspace(SCALE_RANGE[0], SCALE_RANGE[1], 3 * w if n_guesses is None else int(n_guesses))


def correlate(spectrum2, anchor_x, anchor_wavelength, atlas, scales, row_guesses=(), device=None):
    """corr [len(scales)] of the auto-dispersion loop for the given scales, and the filled interpolated rows of `row_guesses`
    (float64 [len(row_guesses), W], or None) -> (corr, rows), NumPy arrays.  ValueError for a scale that is not finite or not
    positive (the kernel's run search assumes x rises with k)."""
    w = int(np.asarray(spectrum2).shape[0])
    if not atlas.first <= anchor_wavelength <= atlas.a_last:
        raise ValueError('anchor wavelength %r lies outside the atlas [%r, %r]' % (anchor_wavelength, atlas.first, atlas.a_last))
    if w < 2:
        raise ValueError('a spectrum of %d pixel(s) has no correlation' % w)
    scales = np.ascontiguousarray(scales, dtype=np.float64)
    bad = np.flatnonzero(~(np.isfinite(scales) & (scales > 0)))
    if bad.size:
        raise ValueError('scale %r (guess %d) is not a finite positive dispersion' % (float(scales[bad[0]]), bad[0]))
    lspec = log_spectrum(spectrum2, anchor_x)
    lo, hi = window(anchor_x, w)
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    sc = torch.from_numpy(scales).to(device)
    corr, run, rows = ops.atlas_correlate(atlas.on(device), atlas.first, atlas.d, anchor_wavelength, anchor_x,
                                          torch.from_numpy(lspec).to(device), lo, hi, sc, row_guesses)
    run = run.cpu().numpy()
    empty = np.flatnonzero(run[:, 0] > run[:, 1])
    if empty.size:
        raise ValueError('no atlas point falls on the %d pixels at dispersion %r (guess %d)' % (w, float(scales[empty[0]]), empty[0]))
    return corr.cpu().numpy(), None if rows is None else rows.cpu().numpy()


def auto_dispersion(spectrum2, anchor_x, anchor_wavelength, atlas, n_guesses=None):
    """The reference's "Auto dispersion" (:271-300) -> (dispersion, corr, scales): the guess of np.linspace(0.02, 0.12, 3 W)
    (n_guesses instead of 3 W if given) whose interpolated atlas correlates best with the log spectrum.  The reference shows
    and stores round(dispersion, 6) but computes shifts with the unrounded value, as shift_for_wavelength should be given."""
    scales = scale_guesses(np.asarray(spectrum2).shape[0], n_guesses)
    corr, _ = correlate(spectrum2, anchor_x, anchor_wavelength, atlas, scales)
    return float(scales[np.argmax(corr)]), corr, scales


def shift_for_wavelength(wavelength, anchor_wavelength, dispersion, fit, iw):
    """The pixel shift that puts `wavelength` on the slit (:245-258) -> (shift, partial).  partial: the shifted line leaves the
    frame on some rows (the reference warns); ValueError when it is outside on every row.  0 <= position <= iw, as the
    reference tests it."""
    if not dispersion > 0:
        raise ValueError('dispersion must be positive')
    shift = int((wavelength - anchor_wavelength) / dispersion)
    positions = shift + np.asarray(fit)[:, 3]
    within = np.logical_and(0 <= positions, positions <= iw)
    if not within.any():
        raise ValueError('line %r (shift %d) is not in the image' % (wavelength, shift))
    return shift, bool(np.logical_not(within).any())


# ---- command line ---------------------------------------------------------------------------------
def _wavelength(text, lines):
    """A wavelength in Angstrom, or a line's name / label from the --lines files."""
    try:
        return float(text)
    except ValueError:
        pass
    for wavelengths, names, labels in lines:
        for i in range(len(names)):
            if text in (names[i], labels[i]):
                return wavelengths[i]
    raise ValueError('%r is neither a wavelength nor a line of the --lines files' % text)


def _parser():
    p = argparse.ArgumentParser(prog='python -m solex_ser_recon_en_amd.spectral',
                                description='Dispersion fit against a solar atlas and the pixel shift of a wavelength.')
    p.add_argument('file', help='SER or AVI scan')
    p.add_argument('--atlas', required=True, help='atlas in alps.npz layout (first, last, step, y)')
    p.add_argument('--anchor', required=True, help='wavelength (A) or line name of the line the scan is centred on')
    p.add_argument('--lines', action='append', default=[], help='line list ("wavelength name" per line); may repeat')
    p.add_argument('--dispersion', type=float, help='A / pixel: skip the fit')
    p.add_argument('--goto', action='append', required=True, help='target wavelength (A) or line name; may repeat')
    p.add_argument('--process', nargs=argparse.REMAINDER,
                   help='then process the scan with these shifts; what follows are SHG_MAIN flags (not -w)')
    return p


def main(argv=None):
    p = _parser()
    args = p.parse_args(sys.argv[1:] if argv is None else list(argv))
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        p.error('the spectral analyser is single-process: run it without torchrun')
    if args.dispersion is not None and not args.dispersion > 0:
        p.error('--dispersion must be positive')
    if args.process and any(a.startswith('-') and 'w' in a for a in args.process):
        p.error('--process takes SHG_MAIN flags other than -w: the shifts come from --goto')
    try:
        lines = [load_lines(f) for f in args.lines]
        anchor = _wavelength(args.anchor, lines)
        targets = [_wavelength(t, lines) for t in args.goto]
    except (OSError, ValueError) as e:
        p.error(str(e))
    if not os.path.isfile(args.file):
        p.error('no such file: %s' % args.file)
    try:
        atlas = load_atlas(args.atlas) if args.dispersion is None else None
    except (OSError, KeyError, ValueError) as e:
        p.error('--atlas: %s' % e)
    res = analyse(args.file)
    try:
        if args.dispersion is None:
            dispersion = auto_dispersion(res['spectrum2'], res['anchor_x'], anchor, atlas)[0]
        else:
            dispersion = args.dispersion
        out = {'anchor_x': res['anchor_x'], 'dispersion': dispersion, 'dispersion_rounded': round(dispersion, 6), 'targets': []}
        for lam in targets:
            shift, partial = shift_for_wavelength(lam, anchor, dispersion, res['fit'], res['iw'])
            if partial:
                warnings.warn('line %r is only partially within the frame' % lam)
            out['targets'].append({'wavelength': lam, 'shift': shift, 'partial': partial})
    except ValueError as e:
        print('error: %s' % e, file=sys.stderr)
        return 1
    print(json.dumps(out), flush=True)
    if args.process is not None:
        from . import CLI_handler, SHG_MAIN, Solex_recon
        opts = SHG_MAIN.default_options()
        shifts = ','.join(str(t['shift']) for t in out['targets'])
        files = CLI_handler.handle_CLI(opts, list(args.process) + ['-w', shifts, args.file])
        Solex_recon.solex_do_work(SHG_MAIN.precheck_files(files, opts), True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
