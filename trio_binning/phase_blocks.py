"""Drop-in alias of :mod:`trio_binning_amd.phase_blocks` (no reference module: the hit tracker is this project's own)."""
import sys as _sys

import trio_binning_amd.phase_blocks as _impl

_sys.modules[__name__] = _impl
