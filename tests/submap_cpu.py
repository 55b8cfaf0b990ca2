"""The numpy float32 restatement of csrc/submap.hip, with the operation order spelled out.  It lives in the
package -- mipsfusion_amd/submap_cpu.py -- because ``SubmapManager(backend="cpu")`` computes its records with it; the tests import
it from here, like the other ``*_cpu.py`` restatements.  The expand rule is not restated: ``expand_rule`` calls the host build of
csrc/submap_dev.h, the header the device compiles."""
from mipsfusion_amd.submap_cpu import *          # noqa: F401,F403
from mipsfusion_amd.submap_cpu import F32, HALF  # noqa: F401
