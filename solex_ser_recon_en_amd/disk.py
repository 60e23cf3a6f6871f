"""What the disk products -- flatten, stack, sharpen, deconvolve (DESIGN.md sections 16 to 20) -- share: a scan's 16-bit disk and its circle
through the pipeline's own stages, and the frame of their command lines: the parse with its refusals, the image written as the
products are, the contrast products."""
import contextlib
import io
import math
import os
import sys

import numpy as np


def host_u(t, dtype):
    """A uint16 / uint32 device tensor as a NumPy array of that type (through the signed type of the same width)."""
    import torch
    signed = {torch.uint16: torch.int16, torch.uint32: torch.int32}[t.dtype]
    return t.view(signed).cpu().numpy().view(dtype)


def scan_disk(file_or_reader, options=None, shift=0, purpose='flattening', dejitter=None):
    """A scan's disk at `shift`: the image _uncontrasted.png shows for that shift before img_rotate -- through the package's own
    stages as Solex_recon.solex_process composes them: line fit, the disks of the ellipse-fit shift and of `shift`, the limb fit,
    the ellipse -> circle warp, transversalium, crop -- and its circle.  -> {'image' (a uint16 device tensor), 'circle' (of the
    image), 'shift', 'ratio', 'phi', 'crop'}.  ValueError for ratio_fixe / slant_fix (no limb fit, hence no circle), de-vignette (a
    float64 frame) and a frame-sharded reader; `purpose` names the caller in the messages ('stacking', 'sharpening').
    dejitter: None, or the keyword arguments of dejitter.measure ({}: its defaults) -- the jitter along the slit is measured on the raw
    disk of the ellipse-fit shift, the one the limb fit reads, every extracted plane is corrected by those shifts before anything
    else sees it, and the record gains 'jitter', measure's."""
    from . import SHG_MAIN, dist
    from .device import DeviceImage, to_device_u16
    from .ellipse_to_circle import correct_image, ellipse_to_circle
    from .fits_io import make_header
    from .Solex_recon import crop_plan, crop_to_width
    from .solex_util import compute_mean_return_fit, correct_transversalium2, extract_disks
    from .video_reader import video_reader
    opts = SHG_MAIN.default_options() if options is None else dict(options)
    if opts['ratio_fixe'] is not None or opts['slant_fix'] is not None:
        raise ValueError('%s needs the limb fit\'s circle: ratio_fixe / slant_fix give none' % purpose)
    if opts['de-vignette']:
        raise ValueError('%s takes the 16-bit disk: de-vignette leaves a float64 one' % purpose)
    opts.update(save_fit=False, flag_display=False, _nolog=True, basefich0='')
    rdr = file_or_reader if hasattr(file_or_reader, 'device_stack') else video_reader(file_or_reader)
    if dist.is_sharded(rdr):
        raise ValueError('%s is single-process: give it the whole scan, not a frame shard' % purpose)
    shift = int(shift)
    ih, iw = int(rdr.ih), int(rdr.iw)
    with contextlib.redirect_stdout(io.StringIO()):               # the stages report on stdout
        _, fit, _, _ = compute_mean_return_fit(rdr, opts, make_header(rdr), iw, ih, '')
        shifts = list(dict.fromkeys([opts['ellipse_fit_shift'], shift]))
        disks, mm = extract_disks(rdr, fit, shifts, flip_x=bool(opts['flip_x']), want_minmax=True)
        jitter = None
        if dejitter is not None:
            from . import dejitter as dj
            jitter = dj.measure(disks[0], **dict(dejitter))
            disks, mm = dj.apply(disks, jitter['shift']), None              # (the cubic overshoots: the extrema are no longer known)
        disk_list = [DeviceImage(disks[i], minmax=None if mm is None else mm[i]) for i in range(len(shifts))]
        own = shifts.index(shift)
        frame, circle, ratio, phi, borders = ellipse_to_circle(disk_list[0], opts, '', need_image=own == 0)
        if own != 0:
            # (solex_process keeps the angle in degrees between the disks, Solex_recon.py:117: the same round trip)
            frame = correct_image(disk_list[own], math.radians(math.degrees(phi)), ratio, np.array([-1.0, -1.0]), -1.0, opts)[0]
        if opts['transversalium']:
            frame = correct_transversalium2(frame, circle, borders, opts, 0, '')
        h, w = to_device_u16(frame).shape
        crop, _ = crop_plan(h, w, circle, opts)
        (frame,), circle_out = crop_to_width([frame], circle, opts)
    res = {'image': to_device_u16(frame), 'circle': tuple(float(v) for v in circle_out), 'shift': shift, 'ratio': float(ratio),
           'phi': float(phi), 'crop': crop}
    if jitter is not None:
        res['jitter'] = jitter
    return res


# ---- --dejitter, the flag the scan products share ----------------------------------------------------
def add_dejitter_argument(p):
    p.add_argument('--dejitter', action='store_true',
                   help='take the scan\'s jitter along the slit out of the raw disks first (dejitter.py; a scan, not a PNG)')


def check_dejitter(p, args, files):
    if args.dejitter and any(f.lower().endswith('.png') for f in files):
        p.error('--dejitter goes with a scan: a PNG has no raw disk to measure')


def jitter_summary(jitter):
    """What a command line prints of dejitter.measure's record."""
    return {'threshold': jitter['threshold'], 'window': jitter['window'], 'n_measured': jitter['n_measured'], 'rms': jitter['rms'],
            'max': jitter['max'], 'line': [jitter['slope'], jitter['intercept']]}


# ---- the frame of the four command lines ------------------------------------------------------------
def parse(p, argv, noun, purpose, checks=None, file_checks=None, png=False, **count):
    """The command line of the product `noun` ('flatten'; `purpose`: 'flattening'): parse, the refusal under torchrun, the caller's
    checks(args), the refusal of -w, then CLI_handler.options_and_files -- `count`: its need, least, most -- with file_checks(args,
    files) before it looks for the files (`png`: a file named .png counts as well, which the SHG_MAIN parser would not know)
    -> (args, opts, files).  Errors exit through p.error."""
    from . import CLI_handler
    args, rest = p.parse_known_args(sys.argv[1:] if argv is None else list(argv))
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        p.error('%s is single-process: run it without torchrun' % purpose)
    if checks is not None:
        checks(args)
    if any(a.startswith('-') and not a.startswith('--') and 'w' in a for a in rest):
        p.error('-w is not a %s flag: give the shift with --shift' % noun)
    pngs = [a for a in rest if png and not a.startswith('-') and a.lower().endswith('.png')]
    opts, files = CLI_handler.options_and_files(p, [a for a in rest if a not in pngs], extra=pngs,
                                                checks=file_checks and (lambda files: file_checks(args, files)), **count)
    return args, opts, files


class _PngHeaderSource:
    """What fits_io.make_header reads of a reader, for an image that came from a PNG."""
    def __init__(self, h, w):
        self.ih, self.iw = h, w


def png_input(path, opts):
    """A 16-bit grey PNG this package wrote as a product's input -> (the uint16 host image, the header source of what is written
    from it, the stem of its outputs); opts['img_rotate'] becomes 0 (a product is already rotated).  ValueError for any other PNG."""
    from .png_io import read_png_gray
    img = read_png_gray(path)
    if img.dtype != np.uint16 or img.ndim != 2:
        raise ValueError('%s is not a 16-bit grey PNG' % path)
    opts['img_rotate'] = 0
    return img, _PngHeaderSource(*img.shape), os.path.splitext(path)[0]


def write_image(image, stem, opts, header_source):
    """The uint16 device image rotated by img_rotate into <stem>.png, and into <stem>.fits (make_header of `header_source`) when
    save_fit -> (the host image as written, the PNG's path, the FITS file's or None)."""
    from .fits_io import make_header, write_fits
    from .png_io import write_png
    from .solex_util import output_path
    host = np.ascontiguousarray(np.rot90(host_u(image.contiguous(), np.uint16), opts['img_rotate'] // 90))
    png, fits = output_path(stem + '.png', opts), None
    write_png(png, host, 0)
    if opts['save_fit']:
        fits = output_path(stem + '.fits', opts)
        write_fits(fits, host, make_header(header_source))
    return host, png, fits


def contrast_products(image, circle, opts, header_source, stem):
    """--contrast: the contrast products of the device image under <stem> (<stem>_clahe.png, ...) -> stem."""
    from . import outputs
    from .fits_io import make_header
    from .solex_util import image_process
    with contextlib.redirect_stdout(sys.stderr):
        image_process(image, circle, opts, make_header(header_source), stem)
        outputs.flush()
    return stem
