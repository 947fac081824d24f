"""astro_amd -- MI355X-native batched lockstep Astro physics.

``BatchedEnv`` (env.py) steps N independent games per GPU through one HIP
kernel (csrc/astro_kernels.hip, C-ABI include/astro_step.h); ``core``
exposes the reference's single-game create/step/play surface on top of it;
``ReplayBuffer`` (replay.py) is the learner's experience replay on the device,
``EpsilonGreedy`` and ``Episodes`` (actor.py) its exploration and per-game
bookkeeping, ``QTrainer`` (train.py) the training loop made of them, ``SGD``,
``RMSprop``, ``Adagrad`` and ``Adam`` (optim.py) its update rules, ``league``
(league.py) the comparison of networks: ``p_better``, ``find_better``,
``compare``, and ``Pool`` / ``tournament`` for many networks on one env,
``Script`` / ``Seats`` for scripted bots with their own arguments per ship and
env block next to them, and ``mutate`` / ``tune_script``, ScriptBot's tuning walk,
``Recorder`` (record.py) whole games of chosen envs recorded on the device, as
the reference's ``Game`` / ``Tick`` logs with the networks' Q values, ``Fork``
(fork.py) env state copied between slots on the device -- ``BatchedEnv.fork_from``,
``snapshot`` and ``restore`` -- and ``Lookahead`` the one-ply search bot on it,
``search`` (search.py) that search's value reduction in one launch,
``Distiller`` (train.py) a Q-network trained on the search's values, and ``es``
(es.py) an antithetic evolution strategy on the packed weights -- ``Population``
and ``ESTrainer``: perturb, play the members on blocks of envs, score, estimate
the gradient, all on the device (csrc/astro_es.hip, include/astro_es.h).
"""
from .config import (Bodies, Config, DEFAULT_CONFIG, Game, SOLO_CONFIG,  # noqa: F401
                     SOLO_EASY_CONFIG, State, Tick, generate_configs)
from .env import BatchedEnv, Observation  # noqa: F401
from .replay import ReplayBuffer  # noqa: F401
from .actor import EpsilonGreedy, Episodes  # noqa: F401
from .optim import SGD, Adagrad, Adam, RMSprop  # noqa: F401
from .train import Distiller, QTrainer  # noqa: F401
from . import league  # noqa: F401
from .league import (Pool, Script, Seats, compare, find_better, mutate, p_better, tournament,  # noqa: F401
                     tune_script)
from . import record  # noqa: F401
from .record import Recorder  # noqa: F401
from . import fork  # noqa: F401
from .fork import Fork, Lookahead  # noqa: F401
from . import search  # noqa: F401
from . import es  # noqa: F401
from .es import ESTrainer, Population  # noqa: F401
