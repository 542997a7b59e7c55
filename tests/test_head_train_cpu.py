"""Training the VGG16 classifier head (05:59-82), the parts that need no GPU:
host-side validation of the new C entry points, fake (meta) kernels of the
new ops, the SGD constructor checks, and two guards of existing behaviour
(Dropout p = 0, no RNG consumed while building a VGG16)."""
import hashlib

import pytest
import torch

import roadrestore as rr

EINVAL, EUNSUPPORTED = -1, -2
A = 4096          # a non-null, 16-byte aligned address; never dereferenced: validation fails first


def test_linear_grads_validate_before_launch():
    L = rr.lib()
    for dt in (0, 1):
        assert L.rr_linear_wgrad(dt, 4, 64, 8, None, A, A, A, 0, None) == EINVAL
        assert L.rr_linear_wgrad(dt, 4, 64, 8, A, None, A, A, 0, None) == EINVAL
        assert L.rr_linear_wgrad(dt, 4, 64, 8, A, A, None, A, 0, None) == EINVAL
        assert L.rr_linear_wgrad(dt, 0, 64, 8, A, A, A, A, 0, None) == EINVAL
        assert L.rr_linear_wgrad(dt, 4, 0, 8, A, A, A, A, 0, None) == EINVAL
        assert L.rr_linear_wgrad(dt, 4, 64, 0, A, A, A, A, 0, None) == EINVAL
        assert L.rr_linear_wgrad(dt, 4, 64, 8, A, A, A + 4, A, 0, None) == EINVAL     # misaligned dw
        assert L.rr_linear_wgrad(dt, 4, 96, 8, A, A, A, A, 0, None) == EUNSUPPORTED   # fin % 64
        assert L.rr_linear_dgrad(dt, 4, 64, 8, None, A, None, A, None) == EINVAL
        assert L.rr_linear_dgrad(dt, 4, 64, 8, A, None, None, A, None) == EINVAL
        assert L.rr_linear_dgrad(dt, 4, 64, 8, A, A, None, None, None) == EINVAL
        assert L.rr_linear_dgrad(dt, 0, 64, 8, A, A, None, A, None) == EINVAL
        assert L.rr_linear_dgrad(dt, 4, 64, 0, A, A, None, A, None) == EINVAL
        assert L.rr_linear_dgrad(dt, 4, 100, 8, A, A, None, A, None) == EUNSUPPORTED
    assert L.rr_linear_wgrad(2, 4, 64, 8, A, A, A, A, 0, None) == EINVAL              # dtype
    assert L.rr_linear_dgrad(7, 4, 64, 8, A, A, None, A, None) == EINVAL


def test_dropout_validates_before_launch():
    L = rr.lib()
    assert L.rr_dropout_fwd(16, 0.5, 1, None, A, A, A, None) == EINVAL
    assert L.rr_dropout_fwd(16, 0.5, 1, A, None, A, A, None) == EINVAL
    assert L.rr_dropout_fwd(16, 0.5, 1, A, A, None, A, None) == EINVAL
    assert L.rr_dropout_fwd(16, 0.5, 1, A, A, A, None, None) == EINVAL
    assert L.rr_dropout_fwd(0, 0.5, 1, A, A, A, A, None) == EINVAL
    assert L.rr_dropout_fwd(16, 1.0, 1, A, A, A, A, None) == EINVAL
    assert L.rr_dropout_fwd(16, -0.1, 1, A, A, A, A, None) == EINVAL
    assert L.rr_dropout_bwd(16, 0.5, None, A, A, None) == EINVAL
    assert L.rr_dropout_bwd(16, 0.5, A, None, A, None) == EINVAL
    assert L.rr_dropout_bwd(16, 0.5, A, A, None, None) == EINVAL
    assert L.rr_dropout_bwd(0, 0.5, A, A, A, None) == EINVAL
    assert L.rr_dropout_mask(16, 0.5, 1, 0, None, None) == EINVAL
    assert L.rr_dropout_mask(0, 0.5, 1, 0, A, None) == EINVAL
    assert L.rr_dropout_mask(16, 0.5, 1, -1, A, None) == EINVAL


def test_cross_entropy_softmax_validate_before_launch():
    L = rr.lib()
    assert L.rr_cross_entropy_workspace(8, 43) >= 8 * 4
    assert L.rr_cross_entropy_workspace(0, 43) == 0
    assert L.rr_cross_entropy(8, 43, None, A, A, None, None, A, 64, None) == EINVAL
    assert L.rr_cross_entropy(8, 43, A, None, A, None, None, A, 64, None) == EINVAL
    assert L.rr_cross_entropy(8, 43, A, A, None, None, None, A, 64, None) == EINVAL
    assert L.rr_cross_entropy(8, 43, A, A, A, None, None, None, 64, None) == EINVAL
    assert L.rr_cross_entropy(0, 43, A, A, A, None, None, A, 64, None) == EINVAL
    assert L.rr_cross_entropy(8, 0, A, A, A, None, None, A, 64, None) == EINVAL
    assert L.rr_cross_entropy(8, 1025, A, A, A, None, None, A, 64, None) == EUNSUPPORTED
    assert L.rr_cross_entropy(8, 43, A, A, A, None, None, A, 4, None) == -4           # workspace
    assert L.rr_softmax_max(8, 43, None, A, A, None) == EINVAL
    assert L.rr_softmax_max(8, 43, A, None, A, None) == EINVAL
    assert L.rr_softmax_max(8, 43, A, A, None, None) == EINVAL
    assert L.rr_softmax_max(0, 43, A, A, A, None) == EINVAL
    assert L.rr_softmax_max(8, 1025, A, A, A, None) == EUNSUPPORTED


def test_sgd_validates_before_launch():
    L = rr.lib()
    assert L.rr_sgd(16, None, A, A, 0.1, 0.9, 0.0, 0.0, 0, 1, None) == EINVAL
    assert L.rr_sgd(16, A, None, A, 0.1, 0.9, 0.0, 0.0, 0, 1, None) == EINVAL
    assert L.rr_sgd(16, A, A, None, 0.1, 0.9, 0.0, 0.0, 0, 1, None) == EINVAL    # momentum, no buffer
    assert L.rr_sgd(0, A, A, A, 0.1, 0.9, 0.0, 0.0, 0, 1, None) == EINVAL
    assert L.rr_sgd(16, A, A, A, 0.1, 0.0, 0.0, 0.0, 1, 1, None) == EINVAL       # nesterov, mu = 0
    assert L.rr_sgd(16, A, A, A, 0.1, 0.9, 0.1, 0.0, 1, 1, None) == EINVAL       # nesterov, dampening
    assert L.rr_sgd_dev(16, A, A, A, None, 0.9, 0.0, 0.0, 0, A, 1, None) == EINVAL
    assert L.rr_sgd_dev(16, A, A, A, A, 0.9, 0.0, 0.0, 0, None, 1, None) == EINVAL
    assert L.rr_sgd_dev(0, A, A, A, A, 0.9, 0.0, 0.0, 0, A, 1, None) == EINVAL
    assert L.rr_sgd_dev(16, None, A, A, A, 0.9, 0.0, 0.0, 0, A, 1, None) == EINVAL


def test_new_ops_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("linear_backward", "dropout", "dropout_backward", "cross_entropy",
                 "cross_entropy_backward", "softmax_max"):
        assert name in rr.layers.OPS
        assert hasattr(torch.ops.rr, name)
    with FakeTensorMode():
        x = torch.empty(5, 192, device="cuda")
        w = torch.empty(43, 192, device="cuda")
        b = torch.empty(43, device="cuda")
        y = torch.ops.rr.linear(x, w, b, 0)
        assert y.shape == (5, 43) and y.dtype == torch.float32
        dx, dw, db = torch.ops.rr.linear_backward(y, x, w, True, 1)
        assert dx.shape == x.shape and dw.shape == w.shape and db.shape == b.shape
        dx, dw, db = torch.ops.rr.linear_backward(y, x, w, False, 0)
        assert dx.numel() == 0 and dw.shape == w.shape
        d, m = torch.ops.rr.dropout(x, 0.5, 1, 0)
        assert d.shape == x.shape and m.shape == x.shape and m.dtype == torch.uint8
        assert torch.ops.rr.dropout_backward(d, m, 0.5).shape == x.shape
        t = torch.empty(5, dtype=torch.int64, device="cuda")
        loss = torch.ops.rr.cross_entropy(y, t)
        assert loss.shape == () and loss.dtype == torch.float32
        assert torch.ops.rr.cross_entropy_backward(loss, y, t).shape == y.shape
        conf, pred = torch.ops.rr.softmax_max(y)
        assert conf.shape == (5,) and conf.dtype == torch.float32
        assert pred.shape == (5,) and pred.dtype == torch.int64


def test_sgd_constructor_checks_and_host_parameters():
    p = torch.nn.Parameter(torch.zeros(3))
    for kw in (dict(lr=-1.0), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-1e-4),
               dict(lr=0.1, nesterov=True), dict(lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)):
        with pytest.raises(ValueError):
            torch.optim.SGD([p], **kw)
        with pytest.raises(ValueError):
            rr.SGD([p], **kw)
    opt = rr.SGD([p], lr=0.1, momentum=0.9)
    assert opt.defaults["momentum"] == 0.9 and opt.defaults["nesterov"] is False
    p.grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="GPU only"):
        opt.step()
    assert rr.CrossEntropyLoss is rr.nn.CrossEntropyLoss


def test_dropout_p0_training_is_identity():
    d = rr.nn.Dropout(0.0)
    d.train()
    x = torch.randn(4, 8)
    assert d(x) is x


def test_vgg16_construction_consumes_no_extra_rng():
    """rr.vgg16() after manual_seed(0) has the initial weights it had before
    Dropout grew a seed and a step counter (checksum recorded on the parent
    commit): Dropout.__init__ draws nothing from torch's generator."""
    torch.manual_seed(0)
    v = rr.vgg16()
    h = hashlib.sha256()
    for _, t in v.state_dict().items():
        h.update(t.numpy().tobytes())
    assert h.hexdigest() == "5e68e07078ccb2f7714464b0dbc8f66627fd7feb6d01dd066fed81edcfe59421"
    # the seed is drawn lazily, at the first training call
    assert all(getattr(m, "seed", None) is None for m in v.classifier if isinstance(m, rr.nn.Dropout))
