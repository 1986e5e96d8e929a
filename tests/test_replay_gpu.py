"""The fused engine's replay caches (engine/fused.py graph() / stepper(), keyed on replay.launch_key of the
launches they hold): a changed argument is never replayed from a stale graph, equal launches are never captured
twice, and invalidate() is the one place that empties both.  40 synthetic images: global batch 16 (here with one
workgroup per sample: by default it, too, would run the split step) is the staged step with a tail of 8, global
batch 8 the split step."""
import pytest
import torch

from csed_514_project_distributed_training_using_pytorch_amd.data import synthetic_mnist
from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer
from csed_514_project_distributed_training_using_pytorch_amd.models import Net
from csed_514_project_distributed_training_using_pytorch_amd.optim import LRSchedule

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def data():
    return synthetic_mnist(40, seed=3)


def _engine(data, global_batch, loopback_world=0, **settings):
    torch.manual_seed(1)
    eng = FusedLeNetTrainer(Net().to(DEV), data, lr=0.05, momentum=0.5, global_batch=global_batch,
                            split=global_batch < 16, loopback_world=loopback_world)
    for name, value in settings.items():
        setattr(eng, name, value)
    eng.set_epoch_order(torch.arange(40))
    return eng


@pytest.mark.parametrize("global_batch", [16, 8])
@pytest.mark.parametrize("name,value", [("train_kernel", 1), ("lr", 0.02)])
def test_changed_argument_gets_its_own_graph_and_executor(data, global_batch, name, value):
    """Setting ``train_kernel`` or ``lr`` after a capture: graph(2) is a new graph that trains like an engine that
    had the setting from the start (2 eager steps, bitwise); setting it back returns the first graph itself,
    cached, not re-captured.  Likewise the native executor.  Before the caches were keyed on the launches'
    arguments the first assertion after the change failed: graph(2) returned the stale graph."""
    eng = _engine(data, global_batch)
    assert (eng.staged, eng.split, eng.grid, eng.tail_size()) == ((True, False, 16, 8) if global_batch == 16
                                                                   else (True, True, 32, 0))
    before = getattr(eng, name)
    g0, st0 = eng.graph(2), eng.stepper()
    assert g0 is not None and eng.graph(2) is g0 and eng.stepper() is st0  # nothing changed: the same ones
    setattr(eng, name, value)
    assert eng.graph(2) is not g0
    eng.run_steps(2)
    torch.cuda.synchronize()
    ref = _engine(data, global_batch, **{name: value})
    ref.step()
    ref.step()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(eng._state(), ref._state())):
        assert torch.equal(a, b), i
    assert eng.step_count.item() == 2
    st1 = eng.stepper()
    assert st1 is not st0 and eng.stepper() is st1
    setattr(eng, name, before)
    assert eng.graph(2) is g0 and len(eng._graphs) == 2
    assert eng.stepper() is not st1
    eng.close()
    ref.close()


def test_equal_length_orders_share_their_graphs_and_another_length_drops_them(data):
    """Two epochs of 2 full steps and a tail of 8: one graph of 2 steps and the tail's graph, captured in the
    first epoch and replayed in the second (2 entries: the count before the keys changed, too)."""
    eng = _engine(data, 16)
    g = torch.Generator().manual_seed(7)
    for _ in range(2):
        eng.train_epoch(torch.randperm(40, generator=g))
    torch.cuda.synchronize()
    assert eng.step_count.item() == 6 and len(eng._graphs) == 2
    eng.stepper()
    eng.set_epoch_order(torch.arange(24))
    assert not eng._graphs and eng._stepper is None
    eng.close()


def test_invalidate_is_what_empties_both_caches(data):
    def warm(eng):
        assert eng.graph(2) is not None and eng.stepper() is not None
        assert eng._graphs and eng._stepper is not None

    def empty(eng):
        return not eng._graphs and eng._stepper is None

    eng = _engine(data, 16)
    warm(eng)
    eng.invalidate()
    assert empty(eng)
    warm(eng)
    eng.load_optimizer_state_dict(eng.optimizer_state_dict())
    assert empty(eng)
    warm(eng)
    eng.set_lr_schedule(LRSchedule(torch.tensor([0.05, 0.02])))
    assert empty(eng)
    warm(eng)
    eng.close()
    assert empty(eng)

    loop = _engine(data, 16, loopback_world=2)
    warm(loop)
    loop.inject_exchange_fault()  # (remaps the pushes behind the same exchange id)
    assert empty(loop)
    loop.inject_exchange_fault(False)
    loop.close()
    assert empty(loop) and loop.exch is None
