"""Host rules of a captured forward (mmmot_amd/modules.py: GraphedForward), without a GPU: which inputs a replay refuses
before it copies anything (check_graph_inputs), what makes a graph stale (graph_stale_reason), and both as __call__
applies them - over CPU tensors, a stub graph and a stub model, then over a real TrackingNet on tests/fake_ops.TorchOps
for every way its packed weights can fall behind its parameters."""
import pytest
import torch

from common import build_model, case_inputs, get_case
from fake_ops import TorchOps
from mmmot_amd.modules import GraphedForward, check_graph_inputs, graph_stale_reason

S, LT, P = 32, 4, 11


def buffers(dtype=torch.float32):
    crops = torch.zeros(LT, 3, S, S) if dtype == torch.float32 else torch.zeros(LT, S, S, 3, dtype=torch.uint8)
    return crops, torch.zeros(P, 3)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def test_matching_inputs_and_none_pass():
    crops, points = buffers()
    check_graph_inputs(crops, points, None, None)                       # None = keep what the buffers hold
    check_graph_inputs(crops, points, torch.ones_like(crops), None)
    check_graph_inputs(crops, points, None, torch.ones_like(points))
    check_graph_inputs(crops, points, crops, points)                    # the buffers themselves
    check_graph_inputs(crops, points, torch.ones(LT, 3, S, 2 * S)[..., ::2], None)  # a strided view: copy_ handles it
    u8, _ = buffers(torch.uint8)
    check_graph_inputs(u8, points, torch.ones_like(u8), points.clone())
    check_graph_inputs(None, points, None, points.clone())              # captured without crops (rows=(1,))
    check_graph_inputs(crops, None, crops.clone(), None)                # captured without points (rows=(0,))


@pytest.mark.parametrize('shape', [(1, 3, S, S), (LT, 1, S, S), (LT, 3, 1, 1), (3, S, S), (S, S), (1,), (),
                                   (LT + 1, 3, S, S), (LT, 3, S, S + 2), (LT, S, S, 3)])
def test_crops_of_another_shape_are_refused(shape):
    """every shape but the last three broadcasts: copy_ would fill the buffer from it without a word"""
    crops, points = buffers()
    with pytest.raises(ValueError, match='crops of a captured forward'):
        check_graph_inputs(crops, points, torch.ones(shape), None)


@pytest.mark.parametrize('shape', [(P, 4), (1, 3), (P, 1), (3,), (P + 1, 3), (P - 1, 3)])
def test_points_of_another_shape_are_refused(shape):
    crops, points = buffers()
    with pytest.raises(ValueError, match='points of a captured forward'):
        check_graph_inputs(crops, points, None, torch.ones(shape))


def test_inputs_of_another_type_are_refused():
    crops, points = buffers()
    u8, _ = buffers(torch.uint8)
    with pytest.raises(ValueError, match='crops of a captured forward'):
        check_graph_inputs(crops, points, torch.ones(LT, 3, S, S, dtype=torch.uint8), None)  # same shape, bytes
    with pytest.raises(ValueError, match='crops of a captured forward'):
        check_graph_inputs(crops, points, torch.ones_like(u8), None)                         # the uint8 layout
    with pytest.raises(ValueError, match='crops of a captured forward'):
        check_graph_inputs(u8, points, torch.ones(LT, S, S, 3), None)                        # floats for a uint8 graph
    with pytest.raises(ValueError, match='crops of a captured forward'):
        check_graph_inputs(u8, points, torch.ones_like(crops), None)
    for dt in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(ValueError, match='crops of a captured forward'):
            check_graph_inputs(crops, points, torch.ones(LT, 3, S, S, dtype=dt), None)
        with pytest.raises(ValueError, match='points of a captured forward'):
            check_graph_inputs(crops, points, None, torch.ones(P, 3, dtype=dt))
    with pytest.raises(ValueError, match='crops of a captured forward'):
        check_graph_inputs(crops, points, [[1.0]], None)                                     # not a tensor


def test_inputs_for_a_buffer_the_graph_does_not_have_are_refused():
    crops, points = buffers()
    with pytest.raises(ValueError, match='captured without crops'):
        check_graph_inputs(None, points, crops, None)
    with pytest.raises(ValueError, match='captured without points'):
        check_graph_inputs(crops, None, None, points)


def test_crops_are_checked_before_points_are_looked_at_and_both_before_any_copy():
    crops, points = buffers()
    with pytest.raises(ValueError, match='points of a captured forward'):
        check_graph_inputs(crops, points, torch.ones_like(crops), torch.ones(P, 4))
    assert not crops.any() and not points.any()


# ---- staleness -------------------------------------------------------------------------------------------------------
def test_stale_reason_truth_table():
    a, b = object(), object()
    assert graph_stale_reason(a, a, 3, 3, False, True) is None
    assert 're-packed' in graph_stale_reason(a, b, 3, 3, False, True)       # another engine
    assert 're-packed' in graph_stale_reason(a, None, 3, 3, False, True)    # invalidated, not rebuilt yet
    assert 're-packed' in graph_stale_reason(a, a, 3, 4, False, True)       # packed tensors replaced under the same engine
    assert 'capture again' in graph_stale_reason(a, a, 3, 3, True, True)    # a training step's device refresh
    why = graph_stale_reason(a, a, 3, 3, False, False)                      # edited in place, nothing re-packed
    assert 'refresh_head()' in why and 'capture again' in why
    assert all(graph_stale_reason(a, e, 3, v, t, c) is not None
               for e in (a, b) for v in (3, 4) for t in (False, True) for c in (False, True)
               if (e, v, t, c) != (a, 3, False, True))                      # any one cause is enough


class StubModel:
    def __init__(self, engine):
        self._engine, self._pack_version, self._trained_since_pack, self.current = engine, 7, False, True

    def _packed_is_current(self):
        return self.current


class StubGraph:
    def __init__(self, owner):
        self.owner, self.replayed = owner, []

    def replay(self):
        self.replayed.append((self.owner.crops.clone(), self.owner.points.clone()))


def stub_graphed():
    eng = object()
    g = object.__new__(GraphedForward)
    g.crops, g.points = buffers()
    g._model, g._engine, g._pack_version = StubModel(eng), eng, 7
    g.graph, g.result = StubGraph(g), 'result'
    return g


def test_call_copies_what_it_is_given_and_keeps_what_it_is_not():
    g = stub_graphed()
    assert not g.stale() and g() == 'result'
    c1, p1 = torch.full((LT, 3, S, S), 1.0), torch.full((P, 3), 2.0)
    g(c1, p1)
    g(None, torch.full((P, 3), 3.0))
    g(torch.full((LT, 3, S, S), 4.0))
    g.crops.fill_(5.0)          # written in place, then replayed without arguments or with the buffers themselves
    g()
    g(g.crops, g.points)
    seen = [(float(c.unique()), float(p.unique())) for c, p in g.graph.replayed]
    assert seen == [(0.0, 0.0), (1.0, 2.0), (1.0, 3.0), (4.0, 3.0), (5.0, 3.0), (5.0, 3.0)]


@pytest.mark.parametrize('bad', ['broadcast', 'dtype', 'points'])
def test_call_refuses_before_it_copies_or_replays(bad):
    g = stub_graphed()
    crops = dict(broadcast=torch.ones(1, 3, S, S), dtype=torch.ones(LT, S, S, 3, dtype=torch.uint8),
                 points=torch.ones(LT, 3, S, S))[bad]
    points = torch.ones(P, 4) if bad == 'points' else torch.ones(P, 3)
    with pytest.raises(ValueError, match='of a captured forward'):
        g(crops, points)
    assert not g.graph.replayed and not g.crops.any() and not g.points.any()


@pytest.mark.parametrize('cause', ['engine', 'version', 'trained', 'edited'])
def test_call_raises_when_stale_and_touches_nothing(cause):
    g = stub_graphed()
    m = g._model
    if cause == 'engine':
        m._engine = object()
    elif cause == 'version':
        m._pack_version += 1
    elif cause == 'trained':
        m._trained_since_pack = True
    else:
        m.current = False
    assert g.stale()
    with pytest.raises(RuntimeError, match='stale'):
        g(torch.ones(LT, 3, S, S), torch.ones(P, 3))
    assert not g.graph.replayed and not g.crops.any() and not g.points.any()


# ---- every staleness cause on a real model (CPU backend; nothing is captured: the rule reads the model only) ---------
def model_and_graph():
    c, base = get_case('s2_C_multiply_none')
    m = build_model(c, base, ops=TorchOps())
    g = object.__new__(GraphedForward)
    g._model, g._engine, g._pack_version = m, m.engine(), m._pack_version
    return c, m, g


@pytest.mark.parametrize('how', ['invalidate', 'set_trunk', 'load_state_dict', 'to', 'set_ops'])
def test_a_repack_makes_the_graph_stale(how):
    c, m, g = model_and_graph()
    assert g.stale_reason() is None
    if how == 'invalidate':
        m.invalidate()
    elif how == 'set_trunk':
        m.set_trunk('f32')
    elif how == 'load_state_dict':
        m.load_state_dict(m.state_dict())
    elif how == 'to':
        m.to('cpu')
    else:
        m.set_ops(TorchOps())
    assert g.stale()
    m.engine()                      # rebuilt: another engine, the graph stays stale
    assert 're-packed' in g.stale_reason()


def test_in_place_edits_make_the_graph_stale_until_what_they_touched_is_packed_again():
    c, m, g = model_and_graph()
    with torch.no_grad():
        m.w_link.conv1[3].weight.mul_(1.001)
    assert 'refresh_head()' in g.stale_reason()                 # a head parameter; _pack_version has not moved
    assert m._pack_version == g._pack_version and m._engine is g._engine
    m.refresh_head()
    assert g.stale_reason() is None                             # packed again in place: the graph follows
    with torch.no_grad():
        m.w_det[1].running_mean.add_(0.01)                      # a head BUFFER (BatchNorm statistics)
    assert g.stale()
    m.refresh_head()
    assert not g.stale()
    with torch.no_grad():
        m.point_net.conv2.weight.mul_(1.001)                    # an encoder parameter
    assert g.stale()
    m.refresh_head()
    assert g.stale(), 'refresh_head() re-packs the heads only'
    with torch.no_grad():
        m(*case_inputs(c))                                      # the eval forward re-packs everything: another engine
    assert 're-packed' in g.stale_reason()


def test_training_makes_the_graph_stale():
    c, m, g = model_and_graph()
    ins = case_inputs(c)
    m.train()
    m.freeze_appearance = True
    m(*ins)                         # one training-mode forward: w_det's BatchNorm buffers took their momentum update
    m.eval()
    assert m._pack_version == g._pack_version and m._engine is g._engine
    assert g.stale() and not m._packed_is_current()
    # the device refresh of a training step (what the next training forward does after optimizer.step())
    c, m, g = model_and_graph()
    with torch.no_grad():
        m.w_link.conv1[3].weight.mul_(1.001)
    m.refresh_head_device()
    assert m._trained_since_pack and g.stale()
    g._pack_version = m._pack_version   # even a graph captured at this very version: the fp16-split copies are stale
    assert m._packed_is_current() and 'training step' in g.stale_reason()
