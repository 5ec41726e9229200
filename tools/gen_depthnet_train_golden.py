"""Generate tests/golden/depthnet_train.npz from the reference's own DepthNet wiring under ``train()`` (development machine only:
it needs the reference checkout that ``oracle.refshim`` loads by path).

Same method as tools/gen_depthnet_golden.py, whose torch restatements of mmdet 2.14's ``BasicBlock`` and mmcv 1.4.0's DCN are put
into the loaded module under those names; the reference's ``DepthNet`` is then run in ``train()`` and float64 with ASPP's dropout
at p = 0.  What it pins is the train-mode wiring: batch statistics in every BatchNorm, the broadcast pooled branch inside
``bn1``'s statistics, the running-statistics update, the gradients torch autograd derives -- not the DCN against mmcv.

Settings (tests/ref_depth_net_train.py): mid = 32, context = 16, depth = 24, 2 cameras, an 8 x 10 map; weights and inputs from
the tests' own seed rule (``seeded_state_dict`` / ``seeded_inputs``), so none are stored.  Stored, all float64: the output, the
running statistics of three BNs after the step, the gradients of six parameters and of the input for the loss sum(out * r).

    python tools/gen_depthnet_train_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

OUT = os.path.join(ROOT, "tests", "golden", "depthnet_train.npz")


def main():
    import gen_depthnet_golden as G
    import ref_depth_net_train as T
    from oracle import refshim
    mod = refshim.install()["lss_bevdepth"]
    mod.BasicBlock, mod.build_conv_layer = G.BasicBlock, G.build_conv_layer
    net = mod.DepthNet(*T.ARGS)
    sd = T.seeded_state_dict(net.state_dict())
    assert len(sd) == 107
    net.load_state_dict(sd, strict=True)
    net = net.double().train()
    net.depth_conv[3].dropout.p = 0.0
    x, mlp, r = T.seeded_inputs()
    xx = x.double().requires_grad_(True)
    out = net(xx, mlp.double())
    (out * r.double()).sum().backward()
    params = dict(net.named_parameters())
    bufs = dict(net.named_buffers())
    arrays = dict(out=out.detach().numpy(), dx=xx.grad.numpy())
    for k in T.GOLDEN_BNS:
        arrays["rm/" + k] = bufs[k + ".running_mean"].numpy()
        arrays["rv/" + k] = bufs[k + ".running_var"].numpy()
        assert int(bufs[k + ".num_batches_tracked"]) == 1
    for k in T.GOLDEN_GRADS:
        arrays["grad/" + k] = params[k].grad.numpy()
    np.savez(OUT, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(arrays), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
