"""MI355X-native vectorised IGLU gridworld: the env.step()/reset() hot path as HIP kernels.

    from gridworld_amd import VecGridWorld          # N envs, tensor obs (the fast path)
    import gridworld_amd; env = gridworld_amd.make('IGLUGridworld-v0', vector_state=True, render=False)
"""
from ._lib import IgwError  # noqa: F401
from .vec_env import SubBatch, VecGridWorld, task_eval  # noqa: F401

__version__ = '0.1.0'
from .env import GridWorld, SizeReward, Wrapper, create_env, make, make_vec, register  # noqa: F401,E402
from .tasks import Task, Tasks, CustomTasks, RandomTasks, Subtasks, dummy_task  # noqa: F401,E402
from . import workloads  # noqa: F401,E402
from . import visualizer  # noqa: F401,E402
from .visualizer import Visualizer, look_at, orbit_poses, render_views  # noqa: F401,E402
from .render import ObsSpec, decode_surface, unproject  # noqa: F401,E402
from . import codec  # noqa: F401,E402
from .codec import encode_jpeg, jpeg_bytes  # noqa: F401,E402
from . import query  # noqa: F401,E402
from .query import ACTION_NAMES as action_mask_names  # noqa: F401,E402
from . import goal  # noqa: F401,E402
from .goal import goal_world  # noqa: F401,E402
from . import aim  # noqa: F401,E402
from .aim import aim_action, aim_decode  # noqa: F401,E402
from . import peek  # noqa: F401,E402
from .peek import peek_best, peek_decode  # noqa: F401,E402
from . import peek_dict  # noqa: F401,E402
from . import vox  # noqa: F401,E402
from .vox import VoxSpec, vox_channel_names  # noqa: F401,E402
from . import worth  # noqa: F401,E402
from .worth import worth_decode, worth_plane_names  # noqa: F401,E402
from . import relabel  # noqa: F401,E402  (the module is callable: G.relabel(...) is relabel.relabel(...))
from .relabel import relabel_future  # noqa: F401,E402
from . import recall  # noqa: F401,E402  (the module is callable: G.recall(...) is recall.recall(...))
