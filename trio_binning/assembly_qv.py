"""Drop-in alias of :mod:`trio_binning_amd.assembly_qv` (no reference module: the database query is this project's own)."""
import sys as _sys

import trio_binning_amd.assembly_qv as _impl

_sys.modules[__name__] = _impl
