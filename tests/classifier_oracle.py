"""darknet19 (yolov2/models/darknet.py:18-29) restated on torch CPU with oracle.models._Ctx (conv + BatchNormalization +
LeakyReLU, MaxPooling2D) and its top -- Conv2D_BN_Leaky(class_num, 1), GlobalAveragePooling2D, Softmax -- plus Keras'
categorical cross-entropy on probabilities. Weights as Model.save_weights writes them ({"<layer>/<index>": array}); unit names
are the repository's (graphs.darknet19_body, "top")."""
import torch

from oracle.models import _Ctx

EPS = 1e-7


def darknet19_forward(weights, x, training=False, unbiased_moving_var=False, leaky_masks=None):
    """(probabilities [N, K], ctx)"""
    c = _Ctx(weights, training, x.dtype, unbiased_moving_var, leaky_masks)

    def cbl(t, name):
        return c.cbl(t, name, bias=True)

    t = cbl(x, "conv1")
    t = c.pool(t, "pool1", 2, 2)
    t = cbl(t, "conv2")
    t = c.pool(t, "pool2", 2, 2)
    for n in ("conv3_1", "conv3_2", "conv3_3"):
        t = cbl(t, n)
    t = c.pool(t, "pool3", 2, 2)
    for n in ("conv4_1", "conv4_2", "conv4_3"):
        t = cbl(t, n)
    t = c.pool(t, "pool4", 2, 2)
    for n in ("conv5_1", "conv5_2", "conv5_3", "conv5_4", "conv5_5"):
        t = cbl(t, n)
    t = c.pool(t, "pool5", 2, 2)
    for n in ("conv6_1", "conv6_2", "conv6_3", "conv6_4", "conv6_5", "top"):
        t = cbl(t, n)
    return torch.softmax(t.mean(dim=(1, 2)), dim=-1), c


def cce(t, p):
    """Keras categorical_crossentropy on probabilities, the mean over the batch (classifier_ref.cce in torch)"""
    q = p / p.sum(dim=1, keepdim=True)
    return (-(t * torch.log(torch.clamp(q, EPS, 1 - EPS))).sum(dim=1)).mean()


def train(weights, x, t, steps, lr=1e-3, unbiased_moving_var=True):
    """`steps` Adam steps (Keras defaults: beta 0.9 / 0.999, epsilon 1e-7) of the float64 oracle on one batch; the moving
    statistics follow the Keras update. Returns the loss of every step (before its update)."""
    w = {k: torch.tensor(v, dtype=torch.float64) for k, v in weights.items()}
    train_keys = [k for k in w if not (k.endswith("_bn/2") or k.endswith("_bn/3"))]
    for k in train_keys:
        w[k].requires_grad_(True)
    opt = torch.optim.Adam([w[k] for k in train_keys], lr=lr, betas=(0.9, 0.999), eps=1e-7)
    xt, tt, losses = torch.tensor(x, dtype=torch.float64), torch.tensor(t, dtype=torch.float64), []
    for _ in range(steps):
        opt.zero_grad()
        p, c = darknet19_forward(w, xt, True, unbiased_moving_var)
        loss = cce(tt, p)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        for name, (mm, mv) in c.moving.items():
            w[f"{name}/2"], w[f"{name}/3"] = mm.detach(), mv.detach()
    return losses
