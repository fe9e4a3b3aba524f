"""The ctypes binding is derived from include/mmmot_hip.h (mmmot_amd/_lib.py: parse_header): one entry of every shape
pinned by literal expectation, and the parser refuses what it does not know instead of guessing."""
from ctypes import POINTER, c_char_p, c_double, c_int, c_long, c_longlong, c_uint, c_ulonglong, c_void_p

import pytest

from mmmot_amd import _lib

S = _lib.SIGNATURES


def test_one_entry_of_every_shape():
    assert S['mmmot_abi_version'] == []
    assert S['mmmot_device_info'] == [c_int, c_void_p, c_char_p, c_int]
    assert S['mmmot_hl16_pack'] == [c_void_p, c_void_p, c_long, c_void_p]
    seq = S['mmmot_associate_sequences']
    assert [i for i, t in enumerate(seq) if t is c_longlong] == [12, 14, 19] and len(seq) == 21
    assert S['mmmot_dropout_mask'] == [c_ulonglong, c_uint, c_long, c_int, c_void_p, c_void_p]
    mot = S['mmmot_clear_mot']
    assert [i for i, t in enumerate(mot) if t is c_double] == [13, 14, 15, 16] and len(mot) == 24
    assert S['mmmot_gemm_rows'] == [POINTER(_lib.GemmArgs), c_void_p]
    assert _lib.DEBUG_SIGNATURES['mmmot_set_patch_variant'] == [c_int]


def test_parameter_records_and_stream_flags():
    assert set(_lib.PARAMS) == set(S)
    for name, params in _lib.PARAMS.items():
        assert [p.ctype for p in params] == S[name]
        last = tuple(params[-1]) if params else None
        assert (name in _lib.TAKES_STREAM) == (last == ('stream', c_void_p, 'void')), name
        assert all(p.name != 'stream' for p in params[:-1]), name
    assert len(_lib.TAKES_STREAM) == 82
    assert tuple(_lib.PARAMS['mmmot_gram_rows'][10]) == ('Gout', c_void_p, 'double')
    assert tuple(_lib.PARAMS['mmmot_u8_normalize'][0]) == ('u8', c_void_p, 'unsigned char')
    assert tuple(_lib.PARAMS['mmmot_trunk_range_bind'][0]) == ('counters4', c_void_p, 'unsigned int')
    assert tuple(_lib.PARAMS['mmmot_absmax'][2]) == ('R', c_long, None)


def test_unknown_types_and_shapes_are_refused():
    with pytest.raises(ValueError, match='mmmot_x'):
        _lib.parse_header('int mmmot_x(short a);')
    with pytest.raises(ValueError, match='mmmot_x'):
        _lib.parse_header('int mmmot_x(float** a, void* stream);')
    with pytest.raises(ValueError, match='mmmot_x'):
        _lib.parse_header('int mmmot_x(const struct nowhere* a);')
    with pytest.raises(ValueError, match='mmmot_gemm_args'):
        _lib.parse_header('typedef struct mmmot_gemm_args { int a, b; } mmmot_gemm_args;')
    structs, params, debug = _lib.parse_header(
        '/* int mmmot_gone(int a); */ typedef struct mmmot_gemm_args { const float* X; int n; } mmmot_gemm_args;\n'
        'int mmmot_x(const mmmot_gemm_args* a, unsigned n, void* stream);\n'
        '#ifdef MMMOT_DEBUG\nint mmmot_y(void);\n#endif\n')
    assert structs['mmmot_gemm_args']._fields_ == [('X', c_void_p), ('n', c_int)]
    assert [p.ctype for p in params['mmmot_x']] == [POINTER(structs['mmmot_gemm_args']), c_uint, c_void_p]
    assert list(params) == ['mmmot_x'] and debug == {'mmmot_y': []}
