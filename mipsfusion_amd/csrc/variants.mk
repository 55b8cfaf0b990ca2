# The variant libraries: ONE translation unit compiled with extra flags and linked with the in-tree objects of all the others
# -> ../variants/libmipsf_<name>.so, the C ABI of the shipped library (`make variants`; loaded by mipsfusion_amd._lib.load).
# One variant = a name in VARIANTS, <name>_UNIT (the unit's stem) and <name>_FLAGS.  tests/hashgrid_cpu.py keeps the same
# constants for the float64 restatement (BUILDS); tests/test_hashgrid_fp64_cpu.py asserts that the two lists agree.
#
# The routed hash-grid scatter: paths of the shipped library that only a batch of more than 2^24 samples, a bin in more than
# eight parts or a 2^22 table reaches, at sizes a test can afford ...
VARIANTS += maskless
maskless_UNIT  = hashgrid
maskless_FLAGS = -DMIPSF_SC_MASKED_MAX_M=1024
VARIANTS += small
small_UNIT  = hashgrid
small_FLAGS = -DMIPSF_SC_MASKED_MAX_M=1024 -DMIPSF_SC_STAGE_CAP=512 -DMIPSF_SC_PART=2048 -DMIPSF_SC_PART_DENSE=1024
VARIANTS += slice10
slice10_UNIT  = hashgrid
slice10_FLAGS = -DMIPSF_SC_MAX_SLICE=1024 -DMIPSF_SC_SLICE_LOG2=10
# ... and the switches hashgrid.hip keeps as the A/B evidence for its defaults
VARIANTS += general
general_UNIT  = hashgrid
general_FLAGS = -DMIPSF_SC_ROUTE_FAST=0
VARIANTS += rt2
rt2_UNIT  = hashgrid
rt2_FLAGS = -DMIPSF_RT_LEVELS=2
VARIANTS += rt4
rt4_UNIT  = hashgrid
rt4_FLAGS = -DMIPSF_RT_LEVELS=4
VARIANTS += interleaved
interleaved_UNIT  = hashgrid
interleaved_FLAGS = -DMIPSF_SC_PLANAR=0
VARIANTS += nostage
nostage_UNIT  = hashgrid
nostage_FLAGS = -DMIPSF_SC_STAGE=0
VARIANTS += agg8
agg8_UNIT  = hashgrid
agg8_FLAGS = -DMIPSF_SC_AGG_MAX=8
VARIANTS += fence
fence_UNIT  = hashgrid
fence_FLAGS = -DMIPSF_SC_PUBLISH_WT=0
VARIANTS += keepzero
keepzero_UNIT  = hashgrid
keepzero_FLAGS = -DMIPSF_SC_SKIP_ZERO=0
VARIANTS += run1
run1_UNIT  = hashgrid
run1_FLAGS = -DMIPSF_SC_RUN=1
VARIANTS += rtb256
rtb256_UNIT  = hashgrid
rtb256_FLAGS = -DMIPSF_RT_BLOCK=256
