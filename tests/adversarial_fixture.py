"""Encoding and layout of tests/golden/adversarial.npz, shared by its generator (tests/golden/gen_goldens_adv.py) and
its readers (tests/test_gpu_adversarial.py, tests/test_adversarial_host.py).

Two cases (image shape, K = 4) x two arms (`dis_consider_image` True / False).  Logits lie on the 1/8 grid in [-6, 6]
and are stored as int8 = 8 * logit (`_i8d8`), the image on the 1/32 grid in [0, 1] as int8 = 32 * value (`_i8d32`):
exact in f32 and in f64.  One discriminator state dict (`sd_<key>`, the reference's `Discriminator(5, HIDDEN)` under
torch seed SEED) serves both arms: the arm without the image drops the image's input channel of `_main.0.weight`.

HIDDEN = 3.  What the file may take (400 KB) decides two things.  (1) Every parameter gradient of four (case, arm)
pairs lies next to the state dict: five times 6 756 floats = 135 KB; hidden_dim = 8 would be five times 44 736 floats
= 895 KB.  The discriminator maps and the BatchNorm row counts (768 / 192 / 48 and 960 / 240 / 60) do not depend on it,
and the channel counts 6 / 12 / 24 take both the 4-byte (C % 4 != 0) and the 16-byte row accesses of the BatchNorm
kernels.  (2) The f64 gradient on the unlabeled logits (49 152 and 61 440 floats per arm, 885 KB in all) is not stored
element by element: the file pins it by its 2-norm, its largest magnitude and PROBES fixed projections
(`probe_vectors`), all f64; a reader recomputes the f64 gradient on the CPU with `replica` (torch's own layers under
the fixture's state dict), checks it against those numbers to 1e-9, and then compares every element against it.

Keys, with <c> a case tag and <a> = img1 / img0:
    <c>_image_i8d32, <c>_lab_i8d8, <c>_unl_i8d8                  inputs
    <c>_<a>_out_lab64, _out_unl64                                discriminator outputs (sigmoid), f64 rounded to f32
    <c>_<a>_gen_loss32, _gen_loss64                              generator_err
    <c>_<a>_gen_g64_norm, _gen_g64_max, _gen_g64_proj            its gradient on the unlabeled logits: 2-norm, max |.|,
                                                                 [PROBES] projections (f64)
    <c>_<a>_dis_loss32, _dis_loss64, _dis_g64_<param>            disc_loss (detached logits) and every parameter gradient
    <c>_<a>_buf64_<buffer>                                       BatchNorm buffers after the step's three forwards
    <c>_<a>_{out,gen,dis,buf}_e_ref                              [2-norm, max, loss] distances of the reference's f32
                                                                 evaluation to its f64 one (the largest over the tensors
                                                                 of the kind; 0 where the kind has no loss)
"""
import numpy as np
import torch
from torch import nn

K = 4
HIDDEN = 3
PROBES = 8
SEED = 11
CASES = {"a": (3, 1, 64, 64), "b": (2, 1, 80, 96)}   # image shapes; maps 32^2 .. 4^2 -> 1x1 and 40x48 .. 5x6 -> 2x3
ARMS = (True, False)                                  # dis_consider_image
BN_ROWS = {"a": (768, 192, 48), "b": (960, 240, 60)}
SCORE_SHAPE = {"a": (3, 1, 1, 1), "b": (2, 1, 2, 3)}
PARAMS = ("_main.0.weight", "_main.2.weight", "_main.3.weight", "_main.3.bias", "_main.5.weight", "_main.6.weight",
          "_main.6.bias", "_main.8.weight", "_main.9.weight", "_main.9.bias", "_main.11.weight")
BUFFERS = tuple(f"_main.{i}.{n}" for i in (3, 6, 9) for n in ("running_mean", "running_var", "num_batches_tracked"))


def arm_tag(consider_image: bool) -> str:
    return f"img{int(consider_image)}"


def decode(name: str, arr: np.ndarray) -> torch.Tensor:
    if name.endswith("_i8d8"):
        return torch.from_numpy(np.asarray(arr)).float() / 8.0
    assert name.endswith("_i8d32"), name
    return torch.from_numpy(np.asarray(arr)).float() / 32.0


def state_dict_of(data, consider_image: bool):
    """the fixture's state dict for an arm: {key: f32 tensor (int64 for the counters)}"""
    sd = {k[len("sd_"):]: torch.from_numpy(np.asarray(data[k])) for k in data.files if k.startswith("sd_")}
    if not consider_image:
        sd["_main.0.weight"] = sd["_main.0.weight"][:, 1:].contiguous()
    return sd


def probe_vectors(n: int) -> torch.Tensor:
    """[PROBES, n] f64: fixed, dense, mutually different directions (closed form: the same numbers everywhere)"""
    i = np.arange(n, dtype=np.float64)
    return torch.from_numpy(np.stack([np.sin(0.37 * (j + 1) * i + j) for j in range(PROBES)]))


def pin(grad64: torch.Tensor):
    """(2-norm, max |.|, projections) of an f64 gradient"""
    g = grad64.detach().double().flatten()
    return float(g.norm()), float(g.abs().max()), (probe_vectors(g.numel()) @ g).numpy()


def replica(sd, consider_image: bool, dtype=torch.float64) -> nn.Sequential:
    """torch's own layers in the discriminator's order under the state dict `sd` (keys `_main.*`), on the CPU"""
    cin, h = (5 if consider_image else K), HIDDEN
    main = nn.Sequential(
        nn.Conv2d(cin, h, 4, 2, 1, bias=False), nn.LeakyReLU(0.2),
        nn.Conv2d(h, 2 * h, 4, 2, 1, bias=False), nn.BatchNorm2d(2 * h), nn.LeakyReLU(0.2),
        nn.Conv2d(2 * h, 4 * h, 4, 2, 1, bias=False), nn.BatchNorm2d(4 * h), nn.LeakyReLU(0.2),
        nn.Conv2d(4 * h, 8 * h, 4, 2, 1, bias=False), nn.BatchNorm2d(8 * h), nn.LeakyReLU(0.2),
        nn.Conv2d(8 * h, 1, 4, 1, 0, bias=False), nn.Sigmoid())
    main.load_state_dict({k[len("_main."):]: v for k, v in sd.items()}, strict=True)
    return main.to(dtype)


def generator_gradient64(sd, consider_image: bool, image, unl):
    """f64 on the CPU: (generator_err, its gradient on the unlabeled logits) of one training-mode forward"""
    dis = replica(sd, consider_image).train()
    z = unl.double().clone().requires_grad_(True)
    p = z.softmax(1)
    out = dis(torch.cat([image.double(), p], 1) if consider_image else p)
    loss = nn.BCELoss()(out, torch.ones_like(out))
    loss.backward()
    return loss.detach(), z.grad


class StoredLogits(torch.nn.Module):
    """a segmentation network stand-in: returns stored logit tensors (leaves that require grad) in turn, whatever it
    is fed; one parameter, so that an optimizer can hold it"""

    def __init__(self, logits, input_dim=1):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.ones(1))
        self.logits = [z.detach().clone().requires_grad_(True) for z in logits]
        self.calls, self._input_dim, self._num_classes = 0, input_dim, logits[0].shape[1]

    num_classes = property(lambda self: self._num_classes)

    def forward(self, x):
        out = self.logits[self.calls % len(self.logits)]
        self.calls += 1
        return out
