"""graph_slam_amd — MI355X-native batch factor-graph optimiser behind the graph_slam C++ surface.

The product is the C-ABI shared library ``libfgo.so`` (``include/fgo.h``): hand-written HIP kernels for
gfx950 + a C++ host.  This Python package is only a ctypes binding used by the tests and ``bench.py``:
``_abi`` declares the library's structs and prototypes and loads it; ``front_end``, ``mapping`` and
``graph`` wrap its calls; ``place`` binds ``include/fgo_place.h`` on its own, and the submodule ``dense`` (not starred in here) ``include/fgo_dense.h``.  There is NO CPU fallback: if the library is missing this import raises, and
if no HIP device is present ``Graph()`` raises.
"""
from ._abi import *                                  # noqa: F401,F403
from ._abi import _HERE, _dp, _i64p, _load           # noqa: F401
from .front_end import *                             # noqa: F401,F403
from .mapping import *                               # noqa: F401,F403
from .place import *                                 # noqa: F401,F403
from .graph import *                                 # noqa: F401,F403
from .graph import _DevArray                         # noqa: F401
from . import dense                                  # noqa: F401,E402  (its names stay in graph_slam_amd.dense)
