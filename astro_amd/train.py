"""The reference trainer's loop (astro/rl.py: QBotTrainer.__call__ / reward /
_step, rl.py:249-328, and train, rl.py:335-374) for a whole ``BatchedEnv``, from
the device pieces: ``env.features`` and ``env.qcontrols`` (astro_qnet.h) with
``actor.EpsilonGreedy`` (astro_actor.h), ``env.step``, ``ReplayBuffer``
(astro_replay.h) and ``QNetwork.sgd_step`` (astro_qtrain.h).

One ``QTrainer.tick()`` is one tick of every env and, once the ring holds
``n_samples`` eligible experiences, ``n_ministeps`` optimisation steps -- the
reference takes them when an n-step window closes, every ``n_steps`` ticks per
bot; with thousands of envs a window closes somewhere on every tick.

Options, all off by default: an ``astro_amd.optim`` update rule instead of
``sgd_step``, a frozen target network for the targets, Double-DQN targets
(astro_qopt.h), and an opponent as ship 1: a scripted bot, a fixed network or a
snapshot of the learner refreshed every K steps (astro_qduel.h).
"""
import torch

from . import actor


class QTrainer:
    """env: the training ``BatchedEnv``; net: a ``qnet.QNetwork``; buf: a
    ``ReplayBuffer`` of the env's shape; explore: an ``actor.EpsilonGreedy`` of
    the env (or None: greedy).  ``seed`` keys the replay sampling; the
    exploration has its own.

    optimizer: an ``astro_amd.optim`` rule (``net.step`` instead of
    ``net.sgd_step(..., lr=lr)``; ``lr`` is then the optimizer's own).
    target_sync (needs an optimizer): the targets come from ``self.target``, a
    frozen ``net.clone()`` -- an int K: hard-copied every K optimisation steps;
    a float in (0, 1): Polyak-averaged with that tau on every step; both inside
    the optimiser's launch.  double: Double-DQN targets (the action the online
    network prefers, valued by the target network).  opponent: 'script',
    'nothing' or 'random' -- ship 1 plays ``env.controls(opponent, seed, t)``
    instead of the network's choice (its experiences still go to the ring:
    Q-learning is off-policy; its exploration state still advances), and ship
    1's Q values are not computed at all.  opponent=<QNetwork>: ship 1 plays
    that fixed network, ``self.rival``, in the same launch that evaluates
    ``net`` for ship 0.  opponent='snapshot' with opponent_sync=K (an int >= 1;
    required with 'snapshot', rejected otherwise): ``self.rival`` is a
    ``net.clone()``, refreshed with ``rival.copy_from(net)`` after every K-th
    optimisation step -- self-play against a frozen copy of oneself.  With a
    network as ship 1 ``explore`` applies to both ships, and both ships'
    experiences go to the ring as before.  opponent='pool' with pool_size=K
    (1..31) and opponent_sync=J: ``self.rivals`` is K clones of ``net``, ship 1
    of the j-th of K blocks of envs plays ``rivals[j]`` (``league.Pool.versus``,
    astro_qpool.h: still one acting launch per tick), and after every J-th
    optimisation step the oldest slot is refreshed with ``copy_from(net)``,
    round robin from slot 0 -- self-play against copies of oneself of K
    different ages.  pool_size=1 is 'snapshot' bit for bit.  pool_size goes with
    'pool' only.  opponent=<league.Script>: ship 1 plays a ScriptBot with those
    arguments.  opponent=<list or tuple> of ``QNetwork``s, ``Script``s and bot
    names: a fixed ladder, ``self.ladder`` -- ship 1 of the j-th of K blocks of
    envs plays ``opponent[j]`` (``league.Seats.versus``: the networks' launch,
    the exploration, then one astro_controls_seats launch, astro_seats.h;
    exploration never alters a scripted seat's control).  ``['script']`` acts as
    'script' does, bit for bit."""

    def __init__(self, env, net, buf, explore, n_samples=1024, n_ministeps=1, lr=1e-2, seed=0,
                 optimizer=None, target_sync=None, double=False, opponent=None, opponent_sync=None, pool_size=None):
        if buf.n_env != env.n_env or buf.nships != env.S:
            raise ValueError('the replay buffer is [%d envs, %d ships], the env [%d, %d]'
                             % (buf.n_env, buf.nships, env.n_env, env.S))
        self.env, self.net, self.buf, self.explore = env, net, buf, explore
        self.n_samples, self.n_ministeps, self.lr, self.seed = int(n_samples), int(n_ministeps), float(lr), int(seed)
        self.nstep = 0     # optimisation steps so far (rl.QNetworkTrainer.nstep)
        self.last = None
        self.optimizer, self.double, self.opponent = optimizer, bool(double), opponent
        self.target, self.sync_every, self.tau = None, None, 1.0
        if target_sync is not None:
            if optimizer is None:
                raise ValueError('target_sync needs an optimizer (the target follows inside its launch)')
            if isinstance(target_sync, int) and not isinstance(target_sync, bool) and target_sync >= 1:
                self.sync_every = target_sync
            elif isinstance(target_sync, float) and 0.0 < target_sync < 1.0:
                self.tau = target_sync
            else:
                raise ValueError('target_sync must be an int >= 1 (steps between hard copies) or a float in (0, 1)')
            self.target = net.clone()
        self.rival, self.rival_every, self.rivals, self.ladder = None, None, None, None
        from .league import Script, Seats
        if isinstance(opponent, (Script, list, tuple)):   # one scripted rival with its own arguments, or a fixed ladder
            if pool_size is not None:
                raise ValueError("pool_size goes with opponent='pool' only")
            if opponent_sync is not None:
                raise ValueError("opponent_sync goes with opponent='snapshot' or 'pool' only")
            if env.S != 2:
                raise ValueError('opponent needs a two-ship env')
            self.ladder = (opponent,) if isinstance(opponent, Script) else tuple(opponent)
            self._acting, self._bot = Seats.versus(env, net, self.ladder), None
            return
        pool = isinstance(opponent, str) and opponent == 'pool'
        if pool_size is not None and not pool:
            raise ValueError("pool_size goes with opponent='pool' only")
        if pool or (isinstance(opponent, str) and opponent == 'snapshot'):
            if not (isinstance(opponent_sync, int) and not isinstance(opponent_sync, bool) and opponent_sync >= 1):
                raise ValueError('opponent=%r needs opponent_sync, an int >= 1 (optimisation steps '
                                 'between refreshes)' % opponent)
            if pool and not (isinstance(pool_size, int) and not isinstance(pool_size, bool) and 1 <= pool_size <= 31):
                raise ValueError("opponent='pool' needs pool_size, an int in [1, 31]")
            if env.S != 2:
                raise ValueError('opponent needs a two-ship env')
            self.rival_every = opponent_sync
            if pool:
                self.rivals = [net.clone() for _ in range(pool_size)]
            else:
                self.rival = net.clone()
        else:
            if opponent_sync is not None:
                raise ValueError("opponent_sync goes with opponent='snapshot' or 'pool' only")
            env._check_opponent(opponent)
            if opponent is not None and not isinstance(opponent, str):
                self.rival = opponent
        # what env.qcontrols takes, and the scripted name whose controls fill ship 1's column
        if pool:
            from .league import Pool
            self._acting, self._bot = Pool.versus(env, net, self.rivals), None
        else:
            self._acting, self._bot = env._with_opponent(net, opponent if self.rival is None else self.rival)

    def _targets(self, r, d, nf, term):
        valuer = self.net if self.target is None else self.target
        return valuer.td_targets(r, d, nf, term, online=self.net) if self.double else valuer.td_targets(r, d, nf, term)

    def _step(self, f, a, targets):
        if self.optimizer is None:
            return self.net.sgd_step(f, a, targets, lr=self.lr)
        follow = self.target
        if self.sync_every is not None and (self.nstep + 1) % self.sync_every != 0:
            follow = None
        return self.net.step(f, a, targets, self.optimizer, target_net=follow, tau=self.tau)

    def tick(self):
        """One tick of acting and (when the ring is ready) training.  Returns
        ``dict(loss=..., n=...)`` like rl.QBotTrainer._step (the summed loss
        of the last ministep as a device scalar, the number of samples as a
        device int32 scalar), or None while the ring fills.  No host
        synchronisation."""
        env, net, buf = self.env, self.net, self.buf
        t = buf.t
        env.features(out=buf.head())
        control = env.qcontrols(self._acting, seed=self.seed, tick0=t, explore=self.explore)   # (seed: a Seats' 'random')
        if self._bot is not None:
            control[:, 1] = env.controls(self._bot, self.seed, t)[:, 1]
        _, reward, done = env.step(control)
        buf.push(control, reward, done)
        if buf.eligible_lower_bound() < self.n_samples:
            return None
        out = None
        for m in range(self.n_ministeps):
            ids = buf.sample(self.n_samples, seed=self.seed, draw=t * self.n_ministeps + m)
            f, a, r, d, nf, term = buf.gather(ids)
            loss = self._step(f, a, self._targets(r, d, nf, term))
            buf.update_loss(ids, loss)
            self.nstep += 1
            if self.rival_every is not None and self.nstep % self.rival_every == 0:
                if self.rivals is None:
                    self.rival.copy_from(net)
                else:   # the oldest slot: round robin from slot 0
                    self.rivals[(self.nstep // self.rival_every - 1) % len(self.rivals)].copy_from(net)
            out = dict(loss=loss.sum(), n=torch.full((), ids.shape[0], dtype=torch.int32, device=loss.device))
        self.last = out
        return out

    def run(self, ticks):
        """``ticks`` calls of ``tick``; returns the last result (or None)."""
        out = None
        for _ in range(int(ticks)):
            out = self.tick()
        return out

    def validate(self, eval_env, games=1, opponent=None, record=None):
        """rl.train's validation (rl.py:352-369): ``eval_env.play_q(net,
        opponent, games)`` with the greedy network from the env's current
        states, as ``actor.Episodes.summary()`` -- the share of games won by
        each ship (ship 0 is the network), the share without a winner and the
        median length in ticks.  opponent: None, a scripted bot's name or a
        ``QNetwork`` (``self.rival``, say) as ship 1.  record: a
        ``record.Recorder`` of ``eval_env`` (see ``play_q``): the games of its
        envs, with the network's Q values, as rl.train saves its validation
        game (rl.py:354-355).  Synchronises."""
        return eval_env._play_q(self.net, opponent, games, None, None, 0, record).summary()
