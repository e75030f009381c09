"""The training loop of the reference (its train.py) on the device: `Trainer` drives `loss.train_step` (one engine call per round:
train.py:111-126) with the batched environment (env.Game) and the planner side of the batch builder
(util.make_batch_dsprites_active_inference), applies the gamma schedule (train.py:101-102) and runs the evaluation block
(train.py:136-173) through `loss.free_energy`; `Trainer.report` is that block and the reward-transition test (train.py:181-186) reduced
on the device (loss.eval_stats) and downloaded once.  tools/train_loop.py is the command line over it.

What a round reads back: nothing of the model's.  `train_step` queues its kernels and writes that round's eight batch statistics
(loss.STEP_MEANS_FIELDS) into one row of a [rounds, 8] device tensor; `epoch()` downloads that tensor once, after the last round.  (The
environment's own validity checks, env.Game.pi_to_action_all / current_frame_nchw, still look at one flag per call, as they do for every
caller, and the planner's first decoder pass behind a step of ModelDown fetches po_net.19.bias, 4 bytes: DESIGN.md section 7g.)

Deviations from the reference, each documented where it applies:
  * gamma lives on the owning ActiveInferenceModel (ModelDown has no gamma: train.py:101 raises AttributeError as shipped), and the Trainer
    keeps gamma, beta_s and beta_o there as Python floats, so that no step has to fetch a 0-d device tensor.  The schedule itself is the
    reference's fp32 arithmetic (a float32 tensor += a Python float), see `next_gamma`.
  * the dSprites archive does not ship: the games run on whatever sprite bank they were built with (env.synthetic_sprite_bank by default).
  * no plots (generate_traversals, reconstructions_plot, stats_plot).  `Trainer.report` produces every number of the epoch report on the
    device (loss.eval_stats), the reward-transition test (train.py:181-186) and the Spearman correlations of generate_traversals.py:36-46
    included, and with `mutual_info=True` that script's mutual_info_regression scores (loss.eval_mutual_info: the estimator as
    scikit-learn defines it for float64 columns).  The Spearman p-values, which the reference computes and drops,
    are not computed."""
import numpy as np
import torch

from . import loss, util
from .loss import OMEGA_PARAMS
from .optim import Adam

# train.py:29-46
DEFAULTS = dict(lr_top=1e-4, lr_mid=1e-4, lr_down=1e-3, deepness=1, samples=1, repeats=5, gamma_rate=0.01, gamma_max=0.8, gamma_delay=30,
                batch=50, rounds=1000, epochs=1000, test_size=1000)
EPOCH_KEYS = loss.STEP_MEANS_FIELDS[:7] + ('omega_last', 'omega_std_last')
EVAL_KEYS = ('F', 'F_top', 'F_mid', 'F_down', 'mse_o', 'kl_div_s', 'kl_div_s_anal', 'kl_div_s_naive', 'kl_div_s_naive_anal', 'omega', 'omega_std',
             'kl_div_pi', 'kl_div_pi_min', 'kl_div_pi_max', 'kl_div_pi_med', 'kl_div_pi_std', 'kl_div_pi_anal', 'var_beta_s', 'var_gamma',
             'var_beta_o', 'var_a', 'var_b', 'var_c', 'var_d', 'TC')
REPORT_KEYS = EVAL_KEYS + ('mse_r', 'spearman')         # what Trainer.report adds: the reward-transition test and the latent-to-factor correlations


def next_gamma(gamma, epoch, gamma_rate=0.01, gamma_max=0.8, gamma_delay=30):
    """train.py:101-102 for one epoch -> the gamma that epoch trains with, a Python float.  The reference's gamma is a float32 tensor:
    the comparison and the increment are fp32 (both Python scalars are rounded to fp32 first), and so are they here."""
    g = np.float32(gamma)
    if epoch > gamma_delay and g < np.float32(gamma_max):
        g = np.float32(g + np.float32(gamma_rate))
    return float(g)


def gamma_at(epoch, gamma0=0.0, gamma_rate=0.01, gamma_max=0.8, gamma_delay=30):
    """the gamma of `epoch` for a run that started at epoch 1 with gamma0 (train.py:100-102)"""
    g = gamma0
    for ep in range(1, epoch + 1):
        g = next_gamma(g, ep, gamma_rate, gamma_max, gamma_delay)
    return g


def total_correlation(data):
    """the total correlation of a Gaussian fitted to the rows of data [n, k]: (sum_k log var_k - log det Cov) / 2 (torchutils.py's
    quantity, which train.py:173 logs), numpy on the host"""
    cov = np.atleast_2d(np.cov(np.asarray(data, dtype=np.float64), rowvar=False))
    return 0.5 * (np.log(np.diag(cov)).sum() - np.linalg.slogdet(cov)[1])


def make_batch_random(games, repeats=5, generator=None):
    """the reference's make_batch_dsprites_random (src/util.py:6-25) with the batched environment, one transition per game: randomise, observe, act on an action drawn
    from a random categorical, observe again -> (o0, o1 [games,1,64,64], pi0 one-hot [games,4]) as device tensors: the evaluation batch"""
    games.randomize_environment_all()
    o0 = games.current_frame_nchw()
    Ppi = torch.rand(games.games_no, 4, device=games.device, generator=generator)
    choice = torch.multinomial(Ppi / Ppi.sum(1, keepdim=True), 1, generator=generator).squeeze(1)
    games.pi_to_action_all(choice, repeats=repeats)
    pi0 = torch.zeros(games.games_no, 4, device=games.device)
    pi0[torch.arange(games.games_no, device=games.device), choice] = 1.0
    return o0, games.current_frame_nchw(), pi0


class Trainer:
    def __init__(self, model, games, optimizers=None, *, lr_top=1e-4, lr_mid=1e-4, lr_down=1e-3, omega_params=OMEGA_PARAMS, deepness=1,
                 samples=1, repeats=5, calc_mean=True, gamma_rate=0.01, gamma_max=0.8, gamma_delay=30, generator=None):
        self.model, self.games = model, games
        if not optimizers:                                  # train.py:89-94
            optimizers = {'top': Adam(model.model_top, lr=lr_top), 'mid': Adam(model.model_mid, lr=lr_mid),
                          'down': Adam(model.model_down, lr=lr_down)}
        loss._step_optimizers(model, optimizers)            # a wrong dict fails here, not in the first round
        self.optimizers = optimizers
        self.omega_params = tuple(float(v) for v in omega_params)
        self.deepness, self.samples, self.repeats, self.calc_mean = int(deepness), int(samples), int(repeats), bool(calc_mean)
        self.gamma_rate, self.gamma_max, self.gamma_delay = float(gamma_rate), float(gamma_max), int(gamma_delay)
        self.generator = generator
        # Python floats from here on (one fetch each, now): train_step then reads no device scalar
        model.gamma, model.beta_s, model.beta_o = float(model.gamma), float(model.beta_s), float(model.beta_o)
        self.means = torch.zeros(0, len(loss.STEP_MEANS_FIELDS), dtype=torch.float32, device=model.device)
        self.rounds_done = 0

    def begin_epoch(self, epoch):
        """train.py:101-102 -> the gamma this epoch trains with (kept on the model as a Python float)"""
        self.model.gamma = next_gamma(self.model.gamma, int(epoch), self.gamma_rate, self.gamma_max, self.gamma_delay)
        return self.model.gamma

    def begin_rounds(self, rounds):
        """a fresh [rounds, 8] statistics tensor: round i writes row i"""
        self.means = torch.zeros(int(rounds), len(loss.STEP_MEANS_FIELDS), dtype=torch.float32, device=self.model.device)
        self.rounds_done = 0

    def round(self):
        """train.py:107-126 -> loss.TrainStep (device tensors; nothing is read back)"""
        if self.rounds_done >= self.means.shape[0]:         # rounds outside epoch(): the tensor grows on the device
            more = torch.zeros(max(1, self.means.shape[0]), self.means.shape[1], dtype=torch.float32, device=self.model.device)
            self.means = torch.cat([self.means, more], 0)
        self.games.randomize_environment_all()
        o0, o1, pi0, log_Ppi = util.make_batch_dsprites_active_inference(self.games, self.model, deepness=self.deepness, samples=self.samples,
                                                                         calc_mean=self.calc_mean, repeats=self.repeats, generator=self.generator)
        out = loss.train_step(self.model, o0, o1, pi0, log_Ppi, self.optimizers, omega_params=self.omega_params,
                              means=self.means[self.rounds_done])
        self.rounds_done += 1
        return out

    def epoch(self, rounds):
        """`rounds` rounds, then ONE download of the statistics -> {EPOCH_KEYS: float}: the average over the rounds of each batch mean
        (kl_pi, omega, F_mid, F_down, nlogpo1, kl_s, kl_naive) and the last round's omega mean / standard deviation (what train.py:158-159
        logs)"""
        self.begin_rounds(rounds)
        for _ in range(int(rounds)):
            self.round()
        m = self.means.cpu().numpy().astype(np.float64)
        out = {k: float(m[:, i].mean()) for i, k in enumerate(loss.STEP_MEANS_FIELDS[:7])}
        out['omega_last'], out['omega_std_last'] = float(m[-1, 1]), float(m[-1, 7])
        return out

    def evaluate(self, o0, o1, pi0):
        """the evaluation block, train.py:136-146, as one free_energy call with omega = var_a / 2 + var_d and log_Ppi = log(pi0 + 1e-15)
        -> {EVAL_KEYS: what train.py:149-173 appends to stats}.  omega / omega_std are the last training round's (train.py:158-159; NaN
        before the first round); TC is computed with numpy on the downloaded qs1."""
        m = self.model
        a, b, c, d = self.omega_params
        pi0 = m._engine.tensor(pi0, (-1, m.pi_dim))
        fe = loss.free_energy(m, o0, o1, pi0, torch.log(pi0 + 1e-15), omega=a / 2.0 + d, omega_params=self.omega_params)
        last = self.means[self.rounds_done - 1].cpu().numpy() if self.rounds_done else np.full(8, np.nan, np.float32)
        kl = fe.kl_pi
        return {
            'F': (fe.F_down + fe.F_mid + fe.F_top).mean().item(), 'F_top': fe.F_top.mean().item(), 'F_mid': fe.F_mid.mean().item(),
            'F_down': fe.F_down.mean().item(), 'mse_o': fe.nlogpo1.mean().item(), 'kl_div_s': fe.kl_s.mean().item(),
            'kl_div_s_anal': fe.kl_s_anal.mean(0).cpu().numpy(), 'kl_div_s_naive': fe.kl_naive.mean().item(),
            'kl_div_s_naive_anal': fe.kl_naive_anal.mean(0).cpu().numpy(), 'omega': float(last[1]), 'omega_std': float(last[7]),
            'kl_div_pi': kl.mean().item(), 'kl_div_pi_min': kl.min().item(), 'kl_div_pi_max': kl.max().item(),
            'kl_div_pi_med': kl.median().item(), 'kl_div_pi_std': kl.std().item(), 'kl_div_pi_anal': fe.kl_pi_anal.mean(0).cpu().numpy(),
            'var_beta_s': float(m.beta_s), 'var_gamma': float(m.gamma), 'var_beta_o': float(m.beta_o), 'var_a': a, 'var_b': b, 'var_c': c,
            'var_d': d, 'TC': float(total_correlation(fe.qs1.cpu().numpy())),
        }

    def report(self, game_test, *, reward_deepness=1, mutual_info=False, n_neighbors=3):
        """The whole per-epoch report, train.py:136-187 without the plots, with ONE download -> {REPORT_KEYS}: EVAL_KEYS as `evaluate` gives
        them, `mse_r` (the reward-transition test, train.py:181-186) and `spearman` [10, 6] (the correlation of every latent of the o0
        sample with every true factor, loss.EVAL_FACTORS: generate_traversals.py:36-46 without the p-values).  On `game_test`: the
        evaluation batch with its true latents, free_energy at omega = var_a / 2 + var_d, the reward-transition batch pushed through
        imagine_future_from_o, and loss.eval_stats over all of it; the last training round's omega mean / std join the row on the device.
        (The environment's own validity checks still look at one flag per call.)  mutual_info=True adds the key `mutual_info` [10, 6]
        behind `spearman`: loss.eval_mutual_info of the same s0 and true factors with device noise (seed: the model's, stage: the rounds
        this trainer has run), written into the same device row, so it is still one download."""
        m = self.model
        a, b, c, d = self.omega_params
        e = m._ready()
        o0, o1, pi0, S0_real, _ = util.make_batch_dsprites_random(game_test, self.repeats, self.generator)
        pi0 = e.tensor(pi0, (-1, m.pi_dim))
        fe = loss.free_energy(m, o0, o1, pi0, torch.log(pi0 + 1e-15), omega=a / 2.0 + d, omega_params=self.omega_params)
        r0, r1, rpi = util.make_batch_dsprites_random_reward_transitions(game_test, deepness=reward_deepness, repeats=self.repeats)
        po1 = m.imagine_future_from_o(r0, rpi)
        n = loss._lib.EFE_EVAL_STATS
        n_mi = loss._lib.EFE_EVAL_MI if mutual_info else 0
        row = torch.full((n + 2 + n_mi,), float('nan'), dtype=torch.float32, device=m.device)
        loss.eval_stats(fe, S0_real, (r1, po1), out=row[:n], engine=e)
        if self.rounds_done:
            row[n:n + 2] = self.means[self.rounds_done - 1][1::6]      # omega, omega_std (STEP_MEANS_FIELDS 1 and 7)
        if mutual_info:
            loss.eval_mutual_info(fe.s0, S0_real, n_neighbors=n_neighbors, seed=m.seed, stage=self.rounds_done, out=row[n + 2:], engine=e)
        h = row.cpu().numpy()
        f = {k: h[s] for k, s in loss.EVAL_STATS_FIELDS.items()}
        var = {'var_beta_s': float(m.beta_s), 'var_gamma': float(m.gamma), 'var_beta_o': float(m.beta_o), 'var_a': a, 'var_b': b, 'var_c': c,
               'var_d': d, 'omega': float(h[n]), 'omega_std': float(h[n + 1])}
        out = {}
        for k in REPORT_KEYS:
            if k in var:
                out[k] = var[k]
            elif k == 'spearman':
                out[k] = f[k].reshape(m.s_dim, len(loss.EVAL_FACTORS)).copy()
            else:
                out[k] = f[k].copy() if f[k].size > 1 else float(f[k][0])
        if mutual_info:
            out['mutual_info'] = h[n + 2:].reshape(m.s_dim, len(loss.EVAL_FACTORS)).copy()
        return out
