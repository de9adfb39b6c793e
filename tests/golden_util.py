"""Load golden fixtures (tests/golden/*.npz, produced by tests/golden/make_golden.py)."""
import contextlib
import glob
import json
import math
import os

import numpy as np
import torch

from oracle import usflows_oracle as orc

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def case_names(small_only=False):
    # (the BASELINE cfg4 fixture -- 1.28 G parameters regenerated from the seed -- is loaded by name in
    # tests/test_configs_gpu.py only: far too big for the per-case loops)
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz"))
                   if not os.path.basename(p).startswith(("grads_", "fit_", "udl_", "image_", "imagegrads_", "imagefit_", "imageradial_", "imageradialfit_", "fitsophia_", "sophia_", "gmfit_", "tbase_", "live_")) and "cfg4" not in p)
    if small_only:
        names = [n for n in names if "d784" not in n]
    return names


def load_case(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    d = json.loads(str(z["spec"]))
    if d["radial_p"] == "inf":
        d["radial_p"] = math.inf
    spec = orc.FlowSpec(**d)
    seed, alpha, family = int(z["seed"]), float(z["alpha"]), str(z["family"])
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    if not sd:  # big model: regenerate from (spec, seed) with the documented generator
        assert family == "synth"
        sd = orc.synth_state_dict(spec, seed=seed, alpha=alpha)
    if "base_distribution.loc" in sd:  # radial loc lives in the state dict
        spec.base_loc = sd["base_distribution.loc"]
    # base loc/scale of laplace/normal cases are part of the generator call; recover them
    # from the fixture name -> kept in make_golden.py; stored alongside for robustness
    arrays = {k: torch.from_numpy(z[k]) for k in z.files
              if k in ("x", "zin", "context", "log_prob32", "log_prob64", "backward32", "backward64",
                       "forward32", "forward64", "total_ladj64", "base_loc", "base_scale")}
    if "base_loc" in arrays:
        spec.base_loc = arrays["base_loc"]
    if "base_scale" in arrays:
        spec.base_scale = arrays["base_scale"]
    return spec, sd, arrays


def gm_live_case_names():
    """the reference's LIVE FLAT configuration (experiments/synthetic/gaussian_mixture.yaml:50-93) for D = 2, 10, 100:
    tests/golden/make_golden_gaussian_mixture.py"""
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "init_d*_k10_gmlive.npz")))


def load_gm_live_grads(name):
    """(loss, log_prior, {parameter: d(-log_prob(x).mean() - log_prior()) / d parameter}) of the reference's fp64 run -- EVERY
    parameter, the GammaMM's and the radial loc included"""
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    return float(z["loss64"]), float(z["log_prior64"]), {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("g/")}


def gm_live_fit_case_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "gmfit_d*_k10_gmlive.npz")))


def load_gm_live_fit(name):
    """(spec, training rows, per-epoch losses, state dict before, state dict after) of the reference's Flow.fit with SophiaG at
    the live hyper-parameters (lr 1e-3, weight_decay 0, batch 32, 2 epochs x 96 rows, shuffle under numpy seed 5)"""
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    d = json.loads(str(z["spec"]))
    spec = orc.FlowSpec(**d)
    sd0 = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd0/")}
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    return spec, torch.from_numpy(z["data"]), [float(v) for v in z["losses"]], sd0, sd


def trainable_base_case_names():
    """flows over the reference's TRAINABLE Laplace / Normal base modules: tests/golden/make_golden_trainable_base.py"""
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "tbase_*.npz")))


def load_trainable_base_case(name):
    """(spec, state dict incl. base_distribution.*, x, log_prob64, loss, {parameter: gradient of -log_prob(x).mean()})"""
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    d = json.loads(str(z["spec"]))
    spec = orc.FlowSpec(**d)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    spec.base_loc = sd["base_distribution.loc"].clone()
    sc = torch.nn.functional.softplus(sd["base_distribution.scale_unconstrained"])
    spec.base_scale = sc.expand(spec.dim).clone() if sc.dim() == 0 else sc.clone()
    return (spec, sd, torch.from_numpy(z["x"]), torch.from_numpy(z["log_prob64"]), float(z["loss64"]),
            {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("g/")})


def grad_case_names():
    """cases with golden GRADIENTS of the training loss from the real reference (tests/golden/make_golden_grads.py)"""
    return sorted(os.path.basename(p)[6:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "grads_*.npz")))


def load_grads(name):
    """(loss, {parameter name: d(-log_prob(x, context).mean()) / d parameter}) of the reference's fp64 run"""
    z = np.load(os.path.join(GOLDEN_DIR, "grads_" + name + ".npz"), allow_pickle=False)
    return float(z["loss"]), {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("g/")}


def fit_case_names():
    """cases with a golden Flow.fit run of the real reference (tests/golden/make_golden_fit.py)"""
    return sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "fit_*.npz")))


def load_fit(name):
    """(training rows, per-epoch losses, state dict after the run) of the reference's Flow.fit:
    2 epochs of SGD(lr=1e-3), batch 32, shuffle=True under numpy seed 5"""
    z = np.load(os.path.join(GOLDEN_DIR, "fit_" + name + ".npz"), allow_pickle=False)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    ps = float(z["prior_scale"]) if "prior_scale" in z.files else -1.0
    return torch.from_numpy(z["data"]), [float(v) for v in z["losses"]], sd, (None if ps < 0 else ps)


def udl_case_names():
    """radial cases with golden UDL profiles of the real reference (tests/golden/make_golden_udl.py)"""
    return sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "udl_*.npz")))


def load_udl(name):
    z = np.load(os.path.join(GOLDEN_DIR, "udl_" + name + ".npz"), allow_pickle=False)
    return dict(q=float(z["q"]), r_max=float(z["r_max"]), n_samples=int(z["n_samples"]),
                cut=torch.from_numpy(z["cut"]), full=torch.from_numpy(z["full"]),
                latent_radius=torch.from_numpy(z["latent_radius"]))


def image_case_names():
    """image-shaped flows of the real reference (tests/golden/make_golden_image.py)"""
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "image_*.npz")))


def load_image_case(name, device="cpu"):
    """(usflows_amd USFlow loaded with the reference's state dict, arrays) of an image-shaped golden case"""
    from usflows_amd.flows import USFlow
    from usflows_amd.networks import ConvNet2D
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    d = json.loads(str(z["spec"]))
    dims = d["in_dims"]
    base = torch.distributions.Laplace(torch.zeros(dims).to(device), torch.ones(dims).to(device))
    flow = USFlow(base, dims, d["coupling_blocks"], ConvNet2D, dict(d["cond_args"]), householder=d["householder"],
                  affine_conjugation=d["affine_conjugation"], masktype=d["masktype"])
    if "synth_seed" in d:
        # parameters regenerated from the seed (tests/image_synth.py: the same call conditioned the reference's flow
        # when the fixture was made; the mirror shares its module structure key for key)
        from image_synth import synth_image_params_
        synth_image_params_(flow, int(d["synth_seed"]))
    else:
        sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
        res = flow.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    if device != "cpu":
        flow = flow.to(device)
    arrays = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("sd/") and k != "spec"}
    return flow, arrays


def image_grad_case_names():
    """image cases with golden gradients of the real reference (tests/golden/make_golden_image_grads.py)"""
    return sorted("image_" + os.path.basename(p)[len("imagegrads_"):-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "imagegrads_*.npz")))


def load_image_grads(name):
    """(loss, {parameter name: d(-log_prob(x).mean()) / d parameter}) of the reference's fp64 run on the case's x"""
    z = np.load(os.path.join(GOLDEN_DIR, "imagegrads_" + name[len("image_"):] + ".npz"), allow_pickle=False)
    return float(z["loss"]), {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("g/")}


def load_image_fit(name):
    """(training rows, per-epoch losses, state dict after the run) of the reference's Flow.fit on an image case:
    2 epochs of SGD(lr=1e-3), batch 32, shuffle=True under numpy seed 5 (fp32 on the CPU)"""
    z = np.load(os.path.join(GOLDEN_DIR, "imagefit_" + name[len("image_"):] + ".npz"), allow_pickle=False)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    return torch.from_numpy(z["data"]), [float(v) for v in z["losses"]], sd


def image_radial_case_names():
    """the reference's LIVE image configurations (radial base with an image-shaped loc, prior_scale 1.0):
    tests/golden/make_golden_image_radial.py"""
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "imageradial_*.npz")))


def image_radial_fit_case_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "imageradialfit_*.npz")))


def build_image_radial_flow(spec, base_sd, device="cpu"):
    """the mirror's USFlow of a live-configuration case: constructor calls as the YAML makes them (mnist.yaml:44-92), layer
    parameters from tests/image_synth.py, the base distribution's stored parameters loaded"""
    from usflows_amd import distributions as D
    from usflows_amd.flows import USFlow
    from usflows_amd.networks import ConvNet2D
    from image_synth import synth_image_params_
    dims = spec["in_dims"]
    torch.manual_seed(spec["seed"])
    if spec["base"] == "lognormal":
        nd = D.LogNormal(loc=torch.ones([1]) * 6, scale=torch.ones([1]) * .35, device="cpu")
    else:
        nd = D.GammaMM(concentration=torch.rand([20]) * 75, rate=torch.rand([20]), mixture_weights=torch.ones([20]) / 20, device="cpu")
    base = D.RadialDistribution(device="cpu", p=float(spec["p"]), loc=torch.zeros(list(dims)), norm_distribution=nd)
    flow = USFlow(base, list(dims), spec["coupling_blocks"], ConvNet2D, dict(spec["cond_args"], c_in=dims[0]),
                  prior_scale=spec["prior_scale"], lu_transform=1, householder=0, affine_conjugation=True, nonlinearity=torch.nn.ReLU())
    synth_image_params_(flow, spec["seed"])
    res = flow.load_state_dict(base_sd, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    if device != "cpu":
        flow = flow.to(device)
    return flow


def load_image_radial_case(name, device="cpu"):
    """(mirror flow, arrays, {parameter name: fp64 gradient of -log_prob(x).mean() - log_prior()}, spec)"""
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    spec = json.loads(str(z["spec"]))
    base_sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    flow = build_image_radial_flow(spec, base_sd, device)
    arrays = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith(("sd/", "g/")) and k != "spec"}
    grads = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("g/")}
    return flow, arrays, grads, spec


def load_image_radial_fit(name, device="cpu"):
    """(mirror flow at the run's start, training rows, per-epoch losses, state dict after the reference's 6 SophiaG steps)"""
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    spec = json.loads(str(z["spec"]))
    base_sd = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd0/")}
    flow = build_image_radial_flow(spec, base_sd, device)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    return flow, torch.from_numpy(z["data"]), [float(v) for v in z["losses"]], sd


def grads_close(named, g_ref, tol=5e-5):
    """the device's fp32 gradients against the reference's fp64 ones: every parameter tensor within ``tol`` of its largest
    entry.  (A ReLU whose input lies within fp32 rounding of zero takes either one-sided derivative, depending on the order of
    evaluation: the gradient fixtures of the deep configurations draw inputs that stay clear of that --
    tests/golden/make_golden_image_radial.py ``kink_margin``; measured round 5: with a pre-activation of 1.4e-7 in the batch
    44 of 75 gradient tensors move by up to 1.7e-4 when the affine runs are composed in another order.)"""
    import torch
    bad = []
    for k, g in g_ref.items():
        assert named[k].grad is not None, k
        got, want = named[k].grad.double().cpu(), torch.as_tensor(g).double().cpu()
        assert got.shape == want.shape, (k, got.shape, want.shape)
        s = max(want.abs().max().item(), 1e-30)
        err = (got - want).abs().max().item() / s
        if err > tol:
            bad.append((err, k))
    assert not bad, f"{len(bad)} of {len(g_ref)} gradients beyond {tol:.0e}: {sorted(bad, reverse=True)[:5]}"


# ---- recorded side-by-side runs of the real reference (tests/golden/live_*.npz, tests/golden/make_golden_live.py) -------
RECORD_LIVE = os.environ.get("USFLOWS_RECORD_LIVE") == "1"
LIVE_THREADS = 4      # torch's intra-op pool while recording and replaying (single-threaded CPU kernels round differently)
_live_store = {}
_live_loaded = {}


class LiveReference:
    """The reference's side of a side-by-side test.  Each result is computed by the live reference while recording
    (USFLOWS_RECORD_LIVE=1, tests/golden/make_golden_live.py) and read from the committed fixture otherwise, so the test
    needs nothing outside the repository.  Keys are "<test id>|<name>"."""

    def __init__(self, fixture, test_id):
        self.fixture, self.prefix = fixture, test_id + "|"
        self.record = RECORD_LIVE

    def _get(self, name, fn, encode, decode):
        key = self.prefix + name
        if self.record:
            v = fn()
            _live_store.setdefault(self.fixture, {})[key] = encode(v)
            return v
        if self.fixture not in _live_loaded:
            with np.load(os.path.join(GOLDEN_DIR, self.fixture + ".npz"), allow_pickle=False) as z:
                _live_loaded[self.fixture] = {k: z[k] for k in z.files}
        return decode(_live_loaded[self.fixture][key])

    def tensor(self, name, fn):
        return self._get(name, fn, lambda v: v.detach().cpu().numpy().copy(), torch.from_numpy)

    def float(self, name, fn):
        """a scalar; None (e.g. the reference raised) is stored as NaN"""
        return self._get(name, fn, lambda v: np.float64("nan" if v is None else float(v)),
                         lambda a: None if math.isnan(float(a)) else float(a))

    def flag(self, name, fn):
        return self._get(name, fn, lambda v: np.bool_(bool(v)), lambda a: bool(a))

    def names(self, name, fn):
        return self._get(name, fn, lambda v: np.array(list(v), dtype=str), lambda a: [str(x) for x in a])

    def shape(self, name, fn):
        return self._get(name, fn, lambda v: np.array(tuple(v), dtype=np.int64), lambda a: tuple(int(x) for x in a))

    def state_dict(self, name, fn):
        keys = self.names(name + "/keys", lambda: list(fn().keys()))
        sd = fn() if self.record else None
        return {k: self.tensor(f"{name}/{k}", lambda k=k: sd[k]) for k in keys}


@contextlib.contextmanager
def live_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(LIVE_THREADS)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def write_recorded_live():
    """(recording only) write what the live reference returned to tests/golden/<fixture>.npz"""
    for fixture, arrays in _live_store.items():
        np.savez_compressed(os.path.join(GOLDEN_DIR, fixture + ".npz"), **arrays)
