"""HipOps checks every tensor it hands to the C-ABI before the entry point is reached: a tensor of another element type
than the header's pointee is a TypeError, a host tensor a RuntimeError - never a launch on reinterpreted bytes."""
import types

import pytest
import torch

from test_kernels_gpu import hip  # noqa: F401  (hip is a fixture)

pytestmark = pytest.mark.gpu


def _t(dtype, device='cuda'):
    return torch.full((8,), -1, dtype=dtype, device=device)


def _cases(hip):
    f, i, u8 = torch.float32, torch.int32, torch.uint8
    tiles = types.SimpleNamespace(row0=_t(i), nrows=_t(i), group=_t(i), T=1)
    # (call, its tensors in argument order with the offending one's place, expected element type)
    return {
        'absmax': (lambda a: hip.absmax(*a), [_t(i), _t(f)], f, i),
        'u8_normalize': (lambda a: hip.u8_normalize(a[0], a[1], a[2], 1, 1), [_t(f), _t(f), _t(f)], u8, f),
        'gram_rows': (lambda a: hip.gram_rows(a[0], 64, a[1], a[2], tiles, a[3], a[4]),
                      [_t(f), _t(f), _t(f), _t(f), _t(torch.float64)], torch.float64, f),
        'track_ids': (lambda a: hip.track_ids(a[0], a[1], a[2], a[3], 1, 4, a[4], a[5]),
                      [_t(f), _t(i), _t(i), _t(i), _t(f), _t(i)], i, f),
        'adam_step_table': (lambda a: hip.adam_step_table(a[0], 1, a[1], 1, 0.9, 0.999, 1e-8), [_t(f), _t(i)], u8, f),
    }


@pytest.mark.parametrize('name', ['absmax', 'u8_normalize', 'gram_rows', 'track_ids', 'adam_step_table'])
def test_wrong_element_type_is_a_type_error_before_any_launch(hip, name):
    call, tensors, want, got = _cases(hip)[name]
    with pytest.raises(TypeError) as e:
        call(tensors)
    assert str(e.value) == 'expected %s, got %s' % (want, got)
    torch.cuda.synchronize()
    assert all(bool((t == -1).all()) for t in tensors)      # nothing ran on them


def test_host_tensor_is_refused(hip):
    out = _t(torch.float32)
    with pytest.raises(RuntimeError, match=r'mmmot_amd HIP ops need device tensors \(got cpu\); there is no CPU fallback'):
        hip.absmax(_t(torch.float32, 'cpu'), out)
    torch.cuda.synchronize()
    assert bool((out == -1).all())
