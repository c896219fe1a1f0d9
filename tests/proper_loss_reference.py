"""Independent float64 torch statement of the two proper-scoring-rule losses for the tests of
bayes_od_rc_amd/proper_losses.py and of the device kernels, and the rows those tests share.

Written from the definitions by another route than the twin: the covariance's Cholesky factor L = A1^-1 diag(exp(ld / 2)) is
built with a triangular solve, the NLL is 0.5 |L^-1 e|^2 + sum log L_kk, the energy score forms the corner-space samples
z_i = T (pb + L n_i) literally, and every gradient is torch.autograd's."""
import numpy as np
import torch

T_CORNERS = torch.tensor([[0, 1, 0, -0.5], [1, 0, -0.5, 0], [0, 1, 0, 0.5], [1, 0, 0.5, 0]], dtype=torch.float64)


def decode(box, anchors):
    """retinanet_model.py:262-285 on rows: (v, u) linear in the anchor, (h, w) through exp clipped to [1e-4, 1e4]."""
    vu = anchors[:, 2:] * box[:, :2] / 10.0 + anchors[:, :2]
    hw = anchors[:, 2:] * torch.clamp(torch.exp(box[:, 2:] / 5.0), 1e-4, 1e4)
    return torch.cat([vu, hw], dim=1)


def cholesky_factor(cov_params):
    """L [n,4,4] with Sigma = L L^T: L = A1^-1 diag(exp(ld / 2)); ld = (c4, c9, c5, c0), A1 rows (1), (c8, 1), (c7, c6, 1),
    (c3, c2, c1, 1)."""
    c = cov_params
    one, zero = torch.ones_like(c[:, 0]), torch.zeros_like(c[:, 0])
    a1 = torch.stack([torch.stack([one, zero, zero, zero], -1), torch.stack([c[:, 8], one, zero, zero], -1),
                      torch.stack([c[:, 7], c[:, 6], one, zero], -1), torch.stack([c[:, 3], c[:, 2], c[:, 1], one], -1)], dim=1)
    half = torch.exp(0.5 * torch.stack([c[:, 4], c[:, 9], c[:, 5], c[:, 0]], -1))
    return torch.linalg.solve_triangular(a1, torch.diag_embed(half), upper=False)


def loss_rows(kind, box, box_t, anchors, cov_params, normals=None):
    """(s_cmp [n], s_reg [n]) as torch tensors of the raw rows; ``normals`` [n,M,4] for kind 5."""
    pb, tb = decode(box, anchors), decode(box_t, anchors)
    L = cholesky_factor(cov_params)
    if kind == 4:
        w = torch.linalg.solve_triangular(L, (pb - tb)[:, :, None], upper=False)[:, :, 0]
        return 0.5 * torch.sum(w * w, dim=1), torch.sum(torch.log(torch.diagonal(L, dim1=1, dim2=2)), dim=1)
    m = normals.shape[1]
    z = (pb[:, None, :] + torch.einsum('nkp,nip->nik', L, normals)) @ T_CORNERS.T
    g = tb @ T_CORNERS.T
    a = torch.linalg.vector_norm(z - g[:, None, :], dim=-1).sum(1)
    b = torch.linalg.vector_norm(z[:, 1:] - z[:, :-1], dim=-1).sum(1)
    return a / m - b / (2.0 * (m - 1)), torch.zeros_like(a)


def autograd_rows(kind, box, box_t, anchors, cov_params, normals=None):
    """(s_cmp, s_reg, d/dbox [n,4], d/dcov_params [n,10]) in NumPy float64: the gradient of sum(s_cmp + s_reg) -- rows are
    independent, so it is every row's own."""
    bx = torch.tensor(np.asarray(box, np.float64), requires_grad=True)
    cv = torch.tensor(np.asarray(cov_params, np.float64), requires_grad=True)
    nn = None if normals is None else torch.tensor(np.asarray(normals, np.float64))
    s_cmp, s_reg = loss_rows(kind, bx, torch.tensor(np.asarray(box_t, np.float64)), torch.tensor(np.asarray(anchors, np.float64)), cv, nn)
    (s_cmp + s_reg).sum().backward()
    return s_cmp.detach().numpy(), s_reg.detach().numpy(), bx.grad.numpy(), cv.grad.numpy()


N_RANDOM = 64
EDGE_NAMES = ("pb_equals_tb", "no_off_diagonals", "ld_plus_8", "ld_minus_8", "p_beyond_upper_clip", "p_beyond_lower_clip", "t_beyond_clip")


def raw_rows(seed=20):
    """64 random rows followed by the planted ones of EDGE_NAMES, as float32 values (what the device takes) in float64
    arrays: box [n,4], box_t [n,4], anchors [n,4] (v, u, h, w), cov_params [n,10]."""
    rng = np.random.default_rng(seed)
    n = N_RANDOM + len(EDGE_NAMES)
    box = rng.normal(0.0, 1.0, (n, 4))
    box_t = rng.normal(0.0, 1.0, (n, 4))
    anchors = np.concatenate([rng.uniform(20.0, 600.0, (n, 2)), rng.uniform(16.0, 256.0, (n, 2))], axis=1)
    cov = rng.normal(0.0, 1.0, (n, 10))
    cov[:, [1, 2, 3, 6, 7, 8]] *= 0.5
    e = N_RANDOM
    box[e] = box_t[e]                                            # pb == tb exactly
    cov[e + 1, [1, 2, 3, 6, 7, 8]] = 0.0
    cov[e + 2, [4, 9, 5, 0]] = 8.0
    cov[e + 3, [4, 9, 5, 0]] = -8.0
    box[e + 4, 2:] = (47.0, 60.0)                                # exp(z / 5) > 1e4
    box[e + 5, 2:] = (-47.0, -60.0)                              # exp(z / 5) < 1e-4
    box_t[e + 6, 2] = 50.0
    return tuple(np.asarray(a, np.float32).astype(np.float64) for a in (box, box_t, anchors, cov))
