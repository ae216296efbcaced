"""One restatement of the attention the kernels of csrc/attention*.hip compute, in plain torch, evaluated in float64 and
float32 (tests/test_attention_matrix_host.py on the CPU, tests/test_attention_matrix.py on the GPU).

Operands as `ops.attention_cm` takes them, channel-major [B, heads * d, L]: q, k, v, the optional positional parts
q_pos / k_pos / k2_pos (concatenated to each head's q / k channels) and the optional second key segment k2 / v2.

  s[b, h, t, s'] = scale * sum_c q[b, h, c, t] k[b, h, c, s']              o = softmax_s'(s) v
  lse[b, h, t]   = log2 sum_s' exp2(scale * log2(e) * s[b, h, t, s'])      (what lc_attention_train_fwd writes)

With `do` among the inputs the case also returns dq, dk, dv for that output gradient, through torch autograd.
`attention_case(...)` builds a `_profile_cases.Case`: `ref32` / `ref64` are (o, lse[, dq, dk, dv]), o and the gradients as
[B, heads, d, L], lse as [B, heads, Lq] -- the form `check_profiles` takes unchanged."""
import math

import torch

from tests._profile_cases import Case

LOG2E = 1.4426950408889634
OPERANDS = ("q", "k", "v", "q_pos", "k_pos", "k2", "k2_pos", "v2")


def heads_of(x, heads):
    """[B, heads * d, L] -> [B, heads, d, L] (a view)."""
    B, C, L = x.shape
    return x.reshape(B, heads, C // heads, L)


def attention(c, heads, scale):
    """c: the operands in ONE dtype (absent or None: not given) -> (o [B, heads, dv, Lq], lse [B, heads, Lq]);
    with c["do"] ([B, heads * dv, Lq]) also dq, dk, dv shaped like the heads of q, k, v."""
    g = lambda n: c.get(n)
    grads = g("do") is not None
    with torch.enable_grad() if grads else torch.no_grad():
        leaves = {n: g(n).clone().requires_grad_() for n in ("q", "k", "v")} if grads else {}
        h = lambda n: None if g(n) is None else heads_of(leaves.get(n, g(n)), heads)
        cat = lambda parts, dim: torch.cat([p for p in parts if p is not None], dim)
        Q = cat([h("q"), h("q_pos")], 2)
        K, V = cat([h("k"), h("k_pos")], 2), h("v")
        if g("k2") is not None:
            K = cat([K, cat([h("k2"), h("k2_pos")], 2)], 3)
            V = cat([V, h("v2")], 3)
        s = torch.einsum("bhct,bhcs->bhts", Q, K) * scale
        lse = torch.logsumexp(s, -1) * LOG2E
        o = torch.einsum("bhts,bhcs->bhct", s.softmax(-1), V)
        if not grads:
            return o, lse
        o.backward(heads_of(g("do"), heads))
    return (o.detach(), lse.detach()) + tuple(heads_of(leaves[n].grad, heads) for n in ("q", "k", "v"))


def attention_case(t, heads, scale):
    """t: seeded float32 operands (see `attention`) -> Case with .heads and .scale."""
    case = Case(dict(t), lambda c: attention(c, heads, scale))
    case.heads, case.scale = heads, scale
    return case


def sdpa(t, heads, scale):
    """torch.nn.functional.scaled_dot_product_attention on the same operands (token-major inside), -> o [B, heads, dv, Lq]."""
    g = lambda n: t.get(n)
    h = lambda n: None if g(n) is None else heads_of(g(n), heads)
    cat = lambda parts, dim: torch.cat([p for p in parts if p is not None], dim)
    Q = cat([h("q"), h("q_pos")], 2)
    K, V = cat([h("k"), h("k_pos")], 2), h("v")
    if g("k2") is not None:
        K = cat([K, cat([h("k2"), h("k2_pos")], 2)], 3)
        V = cat([V, h("v2")], 3)
    o = torch.nn.functional.scaled_dot_product_attention(Q.transpose(2, 3), K.transpose(2, 3), V.transpose(2, 3), scale=scale)
    return o.transpose(2, 3)


def log2_keys(Lk):
    """lse of q = 0: every weight is 1 / Lk."""
    return math.log2(Lk)
