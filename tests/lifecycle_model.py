"""The margin of the create/use/destroy memory tests (tests/test_gpu_lifecycle.py states where the figures come from)."""


CYCLES = 5
PARENT_LARGEST_DROP = 0  # bytes, see above
SMALLEST_BUFFER = 4      # bytes: ws_reg::pass_arrived
MARGIN = PARENT_LARGEST_DROP + SMALLEST_BUFFER
