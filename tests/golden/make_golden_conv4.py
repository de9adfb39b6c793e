"""Golden vectors of image-shaped flows whose conditioners use 4 x 4 convolutions, from the REAL reference (this container
only) -- the models experiments/mnist/mnist_usflow_hyperopt.yaml draws at ``kernel_size: 4``.

    python tests/golden/make_golden_conv4.py     # rewrites tests/golden/conv4/conv4_*.npz

The recipe is tests/golden/make_golden_conv5.py's, run at kernel_size = 4 with padding="same" (torch's placement: one zero before
the image and two after, in each axis) and seeds of its own: the same cases at [16, 7, 7] with 2 coupling blocks, Laplace base,
parameters from tests/image_synth.py,
  (a) conv4_cond_c32   CondConvNet2D(c_in=16, c_hidden=32, num_layers=2, kernel_size=4, padding="same", gating, layer norm),
                       Householder 1, conjugation, soft-training context;
  (b) conv4_cond_c64   the same with c_hidden=64: the 64 -> 64 convolutions stream their weights;
  (c) conv4_plain_c8   an unconditional ConvNet2D, c_hidden=8,
each with log_prob in fp32 and fp64, the layer loop's backward and forward in fp64, with a per-row context and with the implicit
zero context, the fp64 loss, and every parameter's fp64 gradient of -mean(log_prob) rounded to fp32, in ``<case>_grads<i>.npz``
files of at most 400 KB; and the ``fit`` run conv4_fit_plain_c16.npz: the reference's own 2-epoch SGD run of the unconditional
flow at c_hidden=16, with the learning rate chosen by that generator's rule (the first of 1e-3, 1e-4, 1e-5 at which the
reference's fp32 run stays within a tenth of the test's bounds of its own fp64 run; main() prints the figures).  A soft-trained
flow's fit cannot follow a CPU run, for the reason make_golden_conv5.py gives.  Data only."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "conv4")
sys.path.insert(0, HERE)

import make_golden_conv5 as m5  # noqa: E402  (imports the reference through ref_shim; its main() is not run)


def cond_args(c_hidden):
    return dict(c_in=16, c_hidden=c_hidden, num_layers=2, kernel_size=4, padding="same", normalize_layers=True, gating=True)


def main():
    # the 5 x 5 generator's functions read these module globals
    m5.OUT = m5.mgc.OUT = OUT
    m5.cond_args = cond_args
    m5.FIT_NAME, m5.FIT_SEED = "conv4_fit_plain_c16", 64
    m5.mgc.run_case("conv4_cond_c32", m5.DIMS, 2, "CondConvNet2D", cond_args(32), 61)
    m5.mgc.run_case("conv4_cond_c64", m5.DIMS, 2, "CondConvNet2D", cond_args(64), 62)
    m5.run_plain("conv4_plain_c8", 8, 63)
    m5.plain_grads64("conv4_plain_c8", 8, 63)
    for name in ("conv4_cond_c32", "conv4_cond_c64", "conv4_plain_c8"):
        m5.split_grads(name)
    m5.fit_fixture()


if __name__ == "__main__":
    main()
