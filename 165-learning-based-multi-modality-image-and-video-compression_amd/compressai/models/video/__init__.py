from .google import *  # noqa: F401,F403
from .google import __all__  # noqa: F401
