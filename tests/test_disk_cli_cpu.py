"""The refusals the three disk products' command lines share (disk.parse, CLI_handler.options_and_files): every one with the words
it had when each command carried its own copy of the frame.  No GPU: a refusal comes before anything touches one."""
import importlib

import pytest

ONE = 'exactly one SER or AVI file is needed (got %s)'
ONE_OR_PNG = 'exactly one SER, AVI or PNG file is needed (got %s)'
TWO = 'at least two SER or AVI files are needed (got %s)'
MANY = ['scan%02d.ser' % i for i in range(33)]

# (module, argv, WORLD_SIZE, what stderr holds); the exit status is 2 throughout
TABLE = [
    ('flatten', ['a.ser'], '2', 'flattening is single-process: run it without torchrun'),
    ('flatten', ['a.ser', '-w', '3'], None, '-w is not a flatten flag: give the shift with --shift'),
    ('flatten', ['a.ser', '-fw3'], None, '-w is not a flatten flag: give the shift with --shift'),
    ('flatten', [], None, ONE % []),
    ('flatten', ['a.ser', 'b.ser'], None, ONE % ['a.ser', 'b.ser']),
    ('flatten', ['no_such_file.ser'], None, 'no such file: no_such_file.ser'),
    ('flatten', ['a.ser', 'notes.txt'], None, ONE % ['a.ser', 'notes.txt']),
    ('flatten', ['a.png'], None, ONE % ['a.png']),
    ('flatten', ['a.ser', '-r'], None, 'flag -r needs a value'),
    ('flatten', ['a.ser', '--smooth', '2'], None, '--smooth must be odd and >= 1'),
    ('flatten', ['a.ser', '--max-gain', 'nan'], None, '--max-gain must be finite and >= 0'),
    ('stack', ['a.ser', 'b.ser'], '2', 'stacking is single-process: run it without torchrun'),
    ('stack', ['a.ser', 'b.ser', '-w', '3'], None, '-w is not a stack flag: give the shift with --shift'),
    ('stack', [], None, TWO % []),
    ('stack', ['a.ser'], None, TWO % ['a.ser']),
    ('stack', MANY, None, 'at most 32 scans are stacked at a time (got 33)'),
    ('stack', ['a.ser', 'b.ser', '--reference', '2'], None, '--reference must be 0 to 1'),
    ('stack', ['a.ser', 'b.ser', '--reference', '-1'], None, '--reference must be 0 to 1'),
    ('stack', ['no_such_a.ser', 'no_such_b.ser'], None, 'no such file: no_such_a.ser'),
    ('stack', ['a.ser', 'b.ser', 'notes.txt'], None, TWO % ['a.ser', 'b.ser', 'notes.txt']),
    ('stack', ['a.ser', 'b.ser', '-r'], None, 'flag -r needs a value'),
    ('sharpen', ['a.ser'], '2', 'sharpening is single-process: run it without torchrun'),
    ('sharpen', ['a.ser', '-w', '3'], None, '-w is not a sharpen flag: give the shift with --shift'),
    ('sharpen', [], None, ONE_OR_PNG % []),
    ('sharpen', ['a.ser', 'b.ser'], None, ONE_OR_PNG % ['a.ser', 'b.ser']),
    ('sharpen', ['a.ser', 'b.png'], None, ONE_OR_PNG % ['a.ser', 'b.png']),
    ('sharpen', ['no_such_file.ser'], None, 'no such file: no_such_file.ser'),
    ('sharpen', ['no_such_file.png'], None, 'no such file: no_such_file.png'),
    ('sharpen', ['NO_SUCH_FILE.PNG'], None, 'no such file: NO_SUCH_FILE.PNG'),
    ('sharpen', ['a.ser', 'notes.txt'], None, ONE_OR_PNG % ['a.ser', 'notes.txt']),
    ('sharpen', ['a.ser', '-r'], None, 'flag -r needs a value'),
    ('sharpen', ['a.ser', '--circle', '1,2'], None, '--circle is cx,cy,rad'),
    ('sharpen', ['a.ser', '--levels', '7'], None, '--levels is 1 to 6'),
    ('sharpen', ['a.ser', '--gains', '1,1,1', '--levels', '2'], None, 'more --gains or --denoise values than --levels'),
]


@pytest.mark.parametrize('module, argv, world, message', TABLE, ids=['%s-%d' % (row[0], i) for i, row in enumerate(TABLE)])
def test_refusal(monkeypatch, capsys, tmp_path, module, argv, world, message):
    monkeypatch.chdir(tmp_path)                                       # (none of the names is a file here)
    if world is None:
        monkeypatch.delenv('WORLD_SIZE', raising=False)
    else:
        monkeypatch.setenv('WORLD_SIZE', world)
    main = importlib.import_module('solex_ser_recon_en_amd.' + module).main
    with pytest.raises(SystemExit) as exit_info:
        main(argv)
    assert exit_info.value.code == 2
    captured = capsys.readouterr()
    assert message in captured.err
    assert captured.out == ''                                         # stdout is the JSON line's alone
