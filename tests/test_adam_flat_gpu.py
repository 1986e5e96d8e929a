"""optim.FusedAdam and GPU parameters: the per-op engine has no flat Adam kernel, so the optimizer must say so and
touch nothing, not step the parameters with torch kernels (FusedSGD.set_ema's rule)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_fused_adam_refuses_gpu_parameters():
    from csed_514_project_distributed_training_using_pytorch_amd.models import Net
    from csed_514_project_distributed_training_using_pytorch_amd.optim import FusedAdam

    torch.manual_seed(1)
    net = Net().cuda()
    ptrs = [p.data_ptr() for p in net.parameters()]
    with pytest.raises(NotImplementedError, match="CPU parameters only"):
        FusedAdam(net.parameters(), lr=1e-3, decoupled=True)
    assert [p.data_ptr() for p in net.parameters()] == ptrs  # (not re-homed into a flat buffer on the way)
