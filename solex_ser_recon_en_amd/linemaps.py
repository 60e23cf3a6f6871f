"""What the line maps share: the Dopplergram (doppler.py), the line-profile maps (lineprofile.py) and the line-bisector maps
(bisector.py) run through one driver, from a scan to raw maps and to maps in the products' geometry, and one set of command-line
pieces.  Each product module declares only what is its own: the kernel calls, planes, units, file names and FITS keys."""
import argparse
import contextlib
import io
import json
import math
import os
import sys

import numpy as np

C_KM_S = 299792.458
MAX_HALF_WIDTH = 32


def _geometry(rdr, fit, opts):
    """(circle, ratio, phi) exactly as Solex_recon.solex_process obtains them: the limb fit of the ellipse-fit shift's disk (flipped
    with flip_x, as solex_read extracts it), or ratio_fixe / slant_fix with no circle."""
    if opts['ratio_fixe'] is None and opts['slant_fix'] is None:
        from .device import DeviceImage
        from .ellipse_to_circle import ellipse_to_circle
        from .solex_util import extract_disks
        disks, mm = extract_disks(rdr, fit, [opts['ellipse_fit_shift']], flip_x=bool(opts['flip_x']), want_minmax=True)
        disk = DeviceImage(disks[0], minmax=None if mm is None else mm[0])
        with contextlib.redirect_stdout(io.StringIO()):           # ellipse_to_circle reports the borders on stdout
            _, circle, ratio, phi, _ = ellipse_to_circle(disk, opts, '', need_image=False)
        return tuple(float(v) for v in circle), float(ratio), float(phi)
    ratio = opts['ratio_fixe'] if opts['ratio_fixe'] is not None else 1.0
    phi = math.radians(opts['slant_fix']) if opts['slant_fix'] is not None else 0.0
    return (-1, -1, -1), float(ratio), float(phi)


def finish_circle(circle, crop, circle_out):
    """The circle the finish masks with, in the corrected image's columns: the products' circle (crop_plan's circle_out) taken back
    through the crop.  crop_plan centres the crop on int(cx) and moves the circle to the crop's middle column nw // 2, dropping the
    fraction of cx; masking with `circle` itself would put the map's disk that fraction of a pixel off the products' disk."""
    if crop is None or tuple(circle) == (-1, -1, -1):
        return circle
    nw, lo, dx0, n = crop
    return (float(circle_out[0] - dx0 + lo), circle[1], circle[2])


def velocity_factor(dispersion, wavelength):
    """km/s per pixel of shift: (dispersion / wavelength) * c."""
    return (float(dispersion) / float(wavelength)) * C_KM_S


def _line_maps(file_or_reader, options, half_width, display_range, dispersion, wavelength, sharded, measure, finish, shift=None):
    """The driver the three maps share: argument checks, reader (`sharded`: the refusal of a frame-sharded scan), line fit,
    raw = measure(stack, fit, flip_x) and (maps, png) = finish(raw, h00, h01, h02, out_h, out_w, circle, crop) in the products'
    geometry.  A `shift` is refused before the fit when it puts every window outside the frame.  -> (raw, maps, png as NumPy
    arrays, the fields of the result dict all share, km/s per pixel or None)."""
    from . import SHG_MAIN, dist
    from .ellipse_to_circle import _warp_geometry
    from .fits_io import make_header
    from .Solex_recon import crop_plan
    from .solex_util import compute_mean_return_fit
    from .video_reader import video_reader
    if not 1 <= half_width <= MAX_HALF_WIDTH:
        raise ValueError('half_width must lie in [1, %d], got %d' % (MAX_HALF_WIDTH, half_width))
    if not (math.isfinite(display_range) and display_range > 0):
        raise ValueError('display_range must be positive')
    if (dispersion is None) != (wavelength is None):
        raise ValueError('km/s needs both the dispersion and the wavelength')
    if dispersion is not None and not (dispersion > 0 and wavelength > 0):
        raise ValueError('dispersion and wavelength must be positive')
    opts = SHG_MAIN.default_options() if options is None else dict(options)
    opts.update(save_fit=False, flag_display=False, _nolog=True, basefich0='')
    rdr = file_or_reader if hasattr(file_or_reader, 'device_stack') else video_reader(file_or_reader)
    if dist.is_sharded(rdr):
        raise ValueError(sharded)
    ih, iw, n = int(rdr.ih), int(rdr.iw), int(rdr.FrameCount)
    if shift is not None and not 3 - iw - half_width < shift < iw - 3 + half_width:
        raise ValueError('shift %d puts every window outside the frame (%d columns)' % (shift, iw))
    _, fit, _, _ = compute_mean_return_fit(rdr, opts, make_header(rdr), iw, ih, '')
    raw = measure(rdr.device_stack(), fit, bool(opts['flip_x']))
    circle, ratio, phi = _geometry(rdr, fit, opts)
    _, _, mat3, out_h, out_w, _, _ = _warp_geometry(phi, ratio, ih, n)
    crop, circle_out = crop_plan(out_h, out_w, circle, opts)
    maps, png = finish(raw, mat3[0, 0], mat3[0, 1], mat3[0, 2], out_h, out_w, finish_circle(circle, crop, circle_out), crop)
    common = {'circle': circle, 'circle_out': circle_out, 'ratio': ratio, 'phi': phi, 'crop': crop, 'fit': fit, 'half_width': half_width,
              'display_range': float(display_range), 'dispersion': dispersion, 'wavelength': wavelength}
    factor = None if dispersion is None else velocity_factor(dispersion, wavelength)
    return raw.contiguous().cpu().numpy(), maps.cpu().numpy(), png.cpu().numpy(), common, factor


def _km_s(m, factor):
    """A pixel-shift map in km/s."""
    return (m.astype(np.float64) * factor).astype(np.float32)


def _by_plane(res, keys, units, velocity, raw, maps, png, factor, **more):
    """res with raw, maps, png and units as dicts by keys[q] for plane q (the `velocity` keys' maps in km/s given a factor), and
    `more`."""
    units = dict(units)
    out = {key: maps[q] for q, key in enumerate(keys)}
    if factor is not None:
        for key in velocity:
            out[key] = _km_s(out[key], factor)
            units[key] = 'km/s'
    res.update(raw={key: raw[q] for q, key in enumerate(keys)}, maps=out, png={key: png[q] for q, key in enumerate(keys)}, units=units,
               **more)
    return res


# ---- removing the plane a global field (solar rotation) leaves in a shift map ------------------------------------------------
Q_SCALE = 4096                                # shg_map_plane_moments sums q = rint(4096 v)
MAX_CLIP_ITERATIONS = 16


def plane_from_moments(m10):
    """The least-squares plane z = a + b c + g r through the used pixels' z = q / 4096, from shg_map_plane_moments' ten integers {N,
    sum c, sum r, sum c^2, sum c r, sum r^2, sum q, sum q c, sum q r, sum q^2} -> (a, b, g, sigma, n).  Exact rational arithmetic
    (Cramer's rule on Python ints): a, b, g are the exact solution of the 3 x 3 normal equations, each rounded once to float64;
    sigma = sqrt(float(RSS / (N - 3))) with the residual sum of squares exact.  ValueError when N < 4 or the determinant is 0 (the
    used pixels lie on one line)."""
    from fractions import Fraction
    n, sc, sr, scc, scr, srr, sq, sqc, sqr, sqq = (int(v) for v in m10)
    if n < 4:
        raise ValueError('a plane fit needs at least 4 used pixels, got %d' % n)

    def det3(m):
        return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
                + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))

    lhs = ((n, sc, sr), (sc, scc, scr), (sr, scr, srr))
    rhs = (sq, sqc, sqr)
    det = det3(lhs)
    if det == 0:
        raise ValueError('the used pixels lie on one line: no plane through them')
    sol = [Fraction(det3([[rhs[i] if j == k else lhs[i][j] for j in range(3)] for i in range(3)]), det * Q_SCALE) for k in range(3)]
    # at the solution RSS = sum z^2 - a sum z - b sum z c - g sum z r
    rss = Fraction(sqq, Q_SCALE * Q_SCALE) - (sol[0] * sq + sol[1] * sqc + sol[2] * sqr) / Q_SCALE
    return float(sol[0]), float(sol[1]), float(sol[2]), math.sqrt(float(rss / (n - 3))), n


def detrend_plane(m, circle=None, clip=3.0, iterations=3, display_range=None):
    """The map minus its sigma-clipped least-squares plane a + b * column + g * row.  m: a float32 [h, w] GPU tensor, or a NumPy
    array (uploaded; the results then come back as NumPy arrays).  Pass 0 fits every usable pixel (finite, |v| < 64, inside
    `circle` = (cx, cy, r) in the map's own columns and rows; None or (-1, -1, -1): no mask); each of up to `iterations` further
    passes fits the pixels within clip * sigma of the previous plane, and the loop ends early when a pass used the same number of
    pixels as the one before or sigma is 0.  A pass is one launch and an 80-byte readback; the solve is plane_from_moments.
    -> (detrended, png (with display_range R: doppler_finish's display plane of the detrended map) or None, info: a, b, g, sigma,
    n_used, n_valid (pass 0's N), passes, gradient = hypot(b, g), axis_angle_deg = degrees(atan2(g, b)), the direction of steepest
    increase in the (column, row) frame, and with a circle limb_amplitude = gradient * r)."""
    import torch
    from . import ops
    if not (math.isfinite(clip) and clip > 0):
        raise ValueError('clip must be finite and positive')
    if int(iterations) != iterations or not 0 <= iterations <= MAX_CLIP_ITERATIONS:
        raise ValueError('iterations must lie in [0, %d]' % MAX_CLIP_ITERATIONS)
    host = not isinstance(m, torch.Tensor)
    dm = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).cuda() if host else m
    masked = circle is not None and tuple(circle) != (-1, -1, -1)
    slots = torch.empty(10, dtype=torch.int64, device=dm.device)
    a, b, g, sigma, n = plane_from_moments(ops.map_plane_moments(dm, circle, None, slots).cpu().numpy())
    n_valid, passes = n, 1
    for _ in range(int(iterations)):
        if sigma == 0.0:
            break
        before = n
        a, b, g, sigma, n = plane_from_moments(ops.map_plane_moments(dm, circle, (a, b, g, clip * sigma), slots).cpu().numpy())
        passes += 1
        if n == before:
            break
    out, png = ops.map_detrend(dm, (a, b, g), display_range)
    info = {'a': a, 'b': b, 'g': g, 'sigma': sigma, 'n_used': n, 'n_valid': n_valid, 'passes': passes, 'gradient': math.hypot(b, g),
            'axis_angle_deg': math.degrees(math.atan2(g, b))}
    if masked:
        info['limb_amplitude'] = info['gradient'] * float(circle[2])
    if host:
        return out.cpu().numpy(), None if png is None else png.cpu().numpy(), info
    return out, png, info


def disk_stats(res):
    """valid fraction, median and 1st / 99th percentile of the map on the disk (the whole map without a circle)."""
    m = res['map']
    cx, cy, rad = res['circle_out']
    if (cx, cy, rad) == (-1, -1, -1):
        on = np.ones(m.shape, dtype=bool)
    else:
        r = np.arange(m.shape[0], dtype=np.float64)[:, None]
        c = np.arange(m.shape[1], dtype=np.float64)[None, :]
        on = (c - cx) * (c - cx) + (r - cy) * (r - cy) <= rad * rad
    v = m[on]
    v = v[np.isfinite(v)]
    out = {'valid_fraction': float(v.size / max(int(on.sum()), 1))}
    if v.size:
        p1, med, p99 = np.percentile(v.astype(np.float64), [1, 50, 99])
        out.update(median=float(med), p1=float(p1), p99=float(p99))
    else:
        out.update(median=None, p1=None, p99=None)
    return out


# ---- command line ---------------------------------------------------------------------------------
def _parser(prog, usage, description, half_width, helps, shift=False, extra=None):
    """The parser of the flags the CLIs take; helps = the help of --half-width, --range, --dispersion, --wavelength; `shift`:
    --shift / --line after --half-width, then extra(p) adds a CLI's own flags."""
    p = argparse.ArgumentParser(prog=prog, usage=usage, description=description)
    p.add_argument('--half-width', type=int, default=half_width, help=helps[0])
    if shift:
        p.add_argument('--shift', type=int, help='pixel shift of the line to measure (the -w shift; default 0: the fitted line)')
        p.add_argument('--line', type=float, help='A, the line to measure (with --atlas / --anchor: its shift from the analyser)')
    if extra is not None:
        extra(p)
    p.add_argument('--range', type=float, default=2.0, help=helps[1])
    p.add_argument('--dispersion', type=float, help=helps[2])
    p.add_argument('--wavelength', type=float, help=helps[3])
    p.add_argument('--atlas', help='atlas in alps.npz layout: the dispersion from the spectral analyser\'s fit')
    p.add_argument('--anchor', type=float, help='A, the line the scan is centred on (with --atlas)')
    return p


def _cli(p, argv, single, w_flag, extra_checks=None):
    """The command line the CLIs share: parse, validate (`single`, `w_flag`: the refusals under torchrun and of -w; after --range
    the checks of --shift / --line when the parser has them, then extra_checks(args)), the SHG_MAIN flags, the one file and the
    atlas -> (args, opts, path, atlas or None).  Errors exit through p.error."""
    from . import CLI_handler, spectral
    args, rest = p.parse_known_args(sys.argv[1:] if argv is None else list(argv))
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        p.error(single)
    if not 1 <= args.half_width <= MAX_HALF_WIDTH:
        p.error('--half-width must lie in [1, %d]' % MAX_HALF_WIDTH)
    if not (math.isfinite(args.range) and args.range > 0):
        p.error('--range must be positive')
    line = hasattr(args, 'line')
    if line and args.shift is not None and args.line is not None:
        p.error('--shift and --line exclude each other')
    if line and args.line is not None and args.atlas is None:
        p.error('--line needs --atlas and --anchor')
    if extra_checks is not None:
        extra_checks(args)
    if (args.dispersion is None) != (args.wavelength is None):
        p.error('--dispersion and --wavelength go together')
    if (args.atlas is None) != (args.anchor is None):
        p.error('--atlas and --anchor go together')
    if args.atlas is not None and args.dispersion is not None:
        p.error('--atlas / --anchor and --dispersion / --wavelength exclude each other')
    for name in ('dispersion', 'wavelength', 'anchor') + (('line',) if line else ()):
        v = getattr(args, name)
        if v is not None and not (math.isfinite(v) and v > 0):
            p.error('--%s must be positive' % name)
    if any(a.startswith('-') and 'w' in a for a in rest):
        p.error(w_flag)
    opts, (path,) = CLI_handler.options_and_files(p, rest)
    try:
        atlas = spectral.load_atlas(args.atlas) if args.atlas is not None else None
    except (OSError, KeyError, ValueError) as e:
        p.error('--atlas: %s' % e)
    return args, opts, path, atlas


def _cli_dispersion(rdr, opts, args, atlas):
    """(dispersion, wavelength, shift): the flags', or with --atlas / --anchor the analyser's dispersion at the anchor.  With --shift
    / --line in the parser, shift is --shift's (0 by default), or with --line L the analyser's shift of L and L the wavelength; else
    None."""
    from . import spectral
    dispersion, wavelength, a = args.dispersion, args.wavelength, None
    if atlas is not None:
        a = spectral.analyse(rdr, opts)
        dispersion, wavelength = spectral.auto_dispersion(a['spectrum2'], a['anchor_x'], args.anchor, atlas)[0], args.anchor
    if not hasattr(args, 'line'):
        return dispersion, wavelength, None
    if args.line is None:
        return dispersion, wavelength, args.shift or 0
    return dispersion, args.line, spectral.shift_for_wavelength(args.line, args.anchor, dispersion, a['fit'], int(rdr.iw))[0]


def _write_pair(stem, opts, rdr, m, png, units, half_width, dispersion, wavelength, **keys):
    """<stem>.fits (float32 map, header BUNIT, HALFWID, keys, DISPERS / WAVELEN with a dispersion) and <stem>.png (16-bit display
    plane), both rotated by img_rotate -> (fits path, png path, shape written)."""
    from .fits_io import make_header, write_fits
    from .png_io import write_png
    from .solex_util import output_path
    hdr = make_header(rdr)
    hdr['BUNIT'] = units
    hdr['HALFWID'] = half_width
    for k, v in keys.items():
        hdr[k] = v
    if dispersion is not None:
        hdr['DISPERS'] = float(dispersion)
        hdr['WAVELEN'] = float(wavelength)
    k = opts['img_rotate'] // 90
    fits_path, png_path = output_path(stem + '.fits', opts), output_path(stem + '.png', opts)
    m = np.ascontiguousarray(np.rot90(m, k))
    write_fits(fits_path, m, hdr)
    write_png(png_path, np.ascontiguousarray(np.rot90(png, k)), 0)
    return fits_path, png_path, list(m.shape)


def _write_planes(path, opts, rdr, res, dispersion, wavelength, planes, **head):
    """<base>_shift=<S>_<suffix>.{fits,png} of each (name, suffix, key, FITS keys) of `planes` (SHIFT = S in every header) -> the
    JSON line's fields: shape, shift .. wavelength, `head`, then the files, units, median and valid fraction by name."""
    base, shift = os.path.splitext(path)[0], res['shift']
    out = {'shape': None, 'shift': shift, 'half_width': res['half_width'], 'display_range': res['display_range'],
           'dispersion': dispersion, 'wavelength': wavelength, **head, 'fits': {}, 'png': {}, 'units': {}, 'median': {},
           'valid_fraction': {}}
    for name, suffix, key, keys in planes:
        fits_path, png_path, out['shape'] = _write_pair('%s_shift=%d_%s' % (base, shift, suffix), opts, rdr, res['maps'][key],
                                                        res['png'][key], res['units'][key], res['half_width'], dispersion,
                                                        wavelength, **keys, SHIFT=shift)
        stats = disk_stats({'map': res['maps'][key], 'circle_out': res['circle_out']})
        out['fits'][name], out['png'][name], out['units'][name] = fits_path, png_path, res['units'][key]
        out['median'][name], out['valid_fraction'][name] = stats['median'], stats['valid_fraction']
    return out


def _print_json(out, res):
    """Prints the JSON line: `out`, then the geometry (circle, ratio, phi, crop) -> 0, the exit status."""
    out.update(circle=list(res['circle']), ratio=res['ratio'], phi=res['phi'], crop=None if res['crop'] is None else list(res['crop']))
    print(json.dumps(out), flush=True)
    return 0
