"""The build refuses register-resident kernels that a compiler spilled
(wanproxy_amd/build.py: NO_SCRATCH): the reading of hipcc's remarks, on text."""
from wanproxy_amd.build import NO_SCRATCH, SRCS, scratch_of

REMARKS = """\
csrc/xcg_encode_group.hip:30:1: remark: Function Name: _ZN3xcg6smallE
csrc/xcg_encode_group.hip:30:1: remark:     VGPRs: 122
csrc/xcg_encode_group.hip:30:1: remark:     ScratchSize [bytes/lane]: 0
csrc/xcg_encode_group.hip:30:1: warning: failed to meet occupancy target [-Wpass-failed]
csrc/xcg_encode_group.hip:30:1: remark: Function Name: _ZN3xcg6largeE
csrc/xcg_encode_group.hip:30:1: remark:     ScratchSize [bytes/lane]: 112
"""


def test_scratch_is_read_per_kernel():
    assert scratch_of(REMARKS) == {'_ZN3xcg6smallE': 0, '_ZN3xcg6largeE': 112}
    assert scratch_of('no remarks here') == {}


def test_checked_units_are_built():
    assert set(NO_SCRATCH) <= set(SRCS) and 'csrc/xcg_encode_group.hip' in NO_SCRATCH
