from .fused_moe import (fused_experts, fused_moe, fused_topk, grouped_topk,  # noqa: F401
                        invoke_fused_moe_kernel)
from .moe_align_block_size import moe_align_block_size  # noqa: F401
