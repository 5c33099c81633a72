"""Covariance kernels behind the reference's plugin API (ref: gptools/kernel/__init__.py:23-29)."""
from .core import *            # noqa: F401,F403
from .squared_exponential import *   # noqa: F401,F403
from .matern import *          # noqa: F401,F403
from .noise import *           # noqa: F401,F403
from .rational_quadratic import *   # noqa: F401,F403
from .gibbs import *           # noqa: F401,F403
from .warping import *         # noqa: F401,F403
from .masked import *          # noqa: F401,F403
from .periodic import *        # noqa: F401,F403
from .spectral import *        # noqa: F401,F403
