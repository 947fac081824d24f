"""The reference trainer's loop (astro/rl.py: QBotTrainer.__call__ / reward /
_step, rl.py:249-328, and train, rl.py:335-374) for a whole ``BatchedEnv``, from
the device pieces: ``env.features`` and ``env.qcontrols`` (astro_qnet.h) with
``actor.EpsilonGreedy`` (astro_actor.h), ``env.step``, ``ReplayBuffer``
(astro_replay.h) and ``QNetwork.sgd_step`` (astro_qtrain.h).

One ``QTrainer.tick()`` is one tick of every env and, once the ring holds
``n_samples`` eligible experiences, ``n_ministeps`` optimisation steps -- the
reference takes them when an n-step window closes, every ``n_steps`` ticks per
bot; with thousands of envs a window closes somewhere on every tick.
"""
import torch

from . import actor


class QTrainer:
    """env: the training ``BatchedEnv``; net: a ``qnet.QNetwork``; buf: a
    ``ReplayBuffer`` of the env's shape; explore: an ``actor.EpsilonGreedy`` of
    the env (or None: greedy).  ``seed`` keys the replay sampling; the
    exploration has its own."""

    def __init__(self, env, net, buf, explore, n_samples=1024, n_ministeps=1, lr=1e-2, seed=0):
        if buf.n_env != env.n_env or buf.nships != env.S:
            raise ValueError('the replay buffer is [%d envs, %d ships], the env [%d, %d]'
                             % (buf.n_env, buf.nships, env.n_env, env.S))
        self.env, self.net, self.buf, self.explore = env, net, buf, explore
        self.n_samples, self.n_ministeps, self.lr, self.seed = int(n_samples), int(n_ministeps), float(lr), int(seed)
        self.nstep = 0     # optimisation steps so far (rl.QNetworkTrainer.nstep)
        self.last = None

    def tick(self):
        """One tick of acting and (when the ring is ready) training.  Returns
        ``dict(loss=..., n=...)`` like rl.QBotTrainer._step (the summed loss
        of the last ministep as a device scalar, the number of samples as a
        device int32 scalar), or None while the ring fills.  No host
        synchronisation."""
        env, net, buf = self.env, self.net, self.buf
        t = buf.t
        env.features(out=buf.head())
        control = env.qcontrols(net, tick0=t, explore=self.explore)
        _, reward, done = env.step(control)
        buf.push(control, reward, done)
        if buf.eligible_lower_bound() < self.n_samples:
            return None
        out = None
        for m in range(self.n_ministeps):
            ids = buf.sample(self.n_samples, seed=self.seed, draw=t * self.n_ministeps + m)
            f, a, r, d, nf, term = buf.gather(ids)
            loss = net.sgd_step(f, a, net.td_targets(r, d, nf, term), lr=self.lr)
            buf.update_loss(ids, loss)
            self.nstep += 1
            out = dict(loss=loss.sum(), n=torch.full((), ids.shape[0], dtype=torch.int32, device=loss.device))
        self.last = out
        return out

    def run(self, ticks):
        """``ticks`` calls of ``tick``; returns the last result (or None)."""
        out = None
        for _ in range(int(ticks)):
            out = self.tick()
        return out

    def validate(self, eval_env, games=1, opponent=None):
        """rl.train's validation (rl.py:352-369): ``eval_env.play_q(net,
        opponent, games)`` with the greedy network from the env's current
        states, as ``actor.Episodes.summary()`` -- the share of games won by
        each ship (ship 0 is the network), the share without a winner and the
        median length in ticks.  Synchronises."""
        return eval_env._play_q(self.net, opponent, games, None, None, 0).summary()
