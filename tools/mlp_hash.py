"""Fingerprint of the policy kernels' outputs (logits and argmax) on fixed inputs: two library builds
or kernel selections that compute the same sums in the same order print the same digests (A/B parity
check).  Lines, in order:
  * bf16 Medium and Large at 4096 * agents + 37 rows, f32 rows and the fragment-order operand (the
    two lines this tool has always printed: their digests are comparable with older result files);
  * bf16 Small at the same row count rule;
  * precision="f32" Small, Medium and Large, f32 rows (the exact-f32 kernel takes no fragments);
  * all three bf16 variants at WALK_ROWS = 300 * 256 + 37 rows = 301 tasks of 256 rows, more than the
    256 CUs of an MI355X, so 45 persistent workgroups walk a second task (a fixed row count, so the
    digests are comparable across machines).
    WH_MLP_LEGACY=1 python tools/mlp_hash.py   vs   python tools/mlp_hash.py"""
import hashlib
import os
import sys

sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rllib-warehouse_amd")]
import torch  # noqa: E402
import warehouse.policy as wp  # noqa: E402

WALK_ROWS = 300 * 256 + 37
AGENTS = {"small": 4, "medium": 8, "large": 16}


def fragment_operand(rows, in_dim, g):
    """A fragment-order operand (wh_observe_x's layout) of random bf16 of magnitude [0.5, 1)."""
    kq = (in_dim + 2 + 15) // 16
    bits = torch.randint(0, 1 << 15, ((rows + 31) // 32, kq, 64, 8), generator=g, dtype=torch.int32).to("cuda")
    return ((bits & 0x807F) | 0x3F00).to(torch.int16).view(torch.uint8).contiguous()


def digest(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]


def line(variant, rows, precision="bf16", label=None):
    net = wp.MLPPolicy(variant, seed=1, precision=precision)
    g = torch.Generator(device="cpu").manual_seed(5)
    x = (torch.randn((rows, net.in_dim), generator=g) * 4).to("cuda")
    acts, lg = net(x, logits=True, step=0)
    text = f"{label or variant}: rows {digest(lg)} {digest(acts)}"
    if precision == "bf16":
        acts_x, lg_x = net.forward_x(fragment_operand(rows, net.in_dim, g), rows, logits=True, step=0)
        text += f"  fragments {digest(lg_x)} {digest(acts_x)}"
    torch.cuda.synchronize()
    print(text, flush=True)


if __name__ == "__main__":
    for variant in ("medium", "large", "small"):
        line(variant, 4096 * AGENTS[variant] + 37)   # a partial last task
    for variant in ("small", "medium", "large"):
        line(variant, 4096 * AGENTS[variant] + 37, "f32", f"{variant} f32")
    for variant in ("small", "medium", "large"):
        line(variant, WALK_ROWS, label=f"{variant} walk {WALK_ROWS}")
