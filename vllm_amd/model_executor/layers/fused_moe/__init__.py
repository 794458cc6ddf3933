from .fused_moe import fused_experts, invoke_fused_moe_kernel  # noqa: F401
from .moe_align_block_size import moe_align_block_size  # noqa: F401
