"""The case table of the marginal cross-entropy over class groups (afft_softmax_ce_groups, csrc/loss.hip) and what its tests share:
the smallest shapes at which a kernel of one 256-thread workgroup per row, groups strided over its four waves and a group's members
over a wave's 64 lanes, can go wrong.  Everything here is CPU tensors; `launch` puts one case on the device.

A case: x [rows, C], group_of [C], G, `glabels` (hard) and `gsoft` (soft) group targets for the same rows, keep or None, gscale, row_g
or None.  None of the cases in CASES holds a bad row (BAD_CASES do)."""
import torch

from ce_cases import SENT, dev, to_dev

F32 = torch.float32


def gen(seed):
    return torch.Generator().manual_seed(seed)


def random_map(C, G, g, ungrouped=0.0):
    """a map in which every group has a member (C >= G): a permutation's first G classes seed the groups, the others draw one"""
    perm = torch.randperm(C, generator=g)
    go = torch.randint(0, G, (C,), generator=g)
    go[perm[:G]] = torch.arange(G)
    if ungrouped:
        rest = perm[G:]
        go[rest[torch.rand(rest.numel(), generator=g) < ungrouped]] = -1
    return go


def sized_map():
    """C = 400: group 0 has 1 member, group 1 has 65 (the lane stride's second trip), group 2 has 300 (its fifth), group 3 is EMPTY,
    the other 34 classes are in no group; the classes are interleaved, not in blocks"""
    go = torch.cat([torch.tensor([0]), torch.full((65,), 1), torch.full((300,), 2), torch.full((34,), -1)])
    return go[torch.randperm(400, generator=gen(11))], 4


def targets(rows, G, g, allowed=None):
    """hard labels over the allowed groups (every one of them used when rows allow) and soft targets with exact zeros among them"""
    allowed = torch.arange(G) if allowed is None else torch.as_tensor(allowed)
    glabels = allowed[torch.arange(rows) % allowed.numel()][torch.randperm(rows, generator=g)]
    soft = torch.zeros(rows, G)
    w = torch.rand(rows, allowed.numel(), generator=g) * (torch.rand(rows, allowed.numel(), generator=g) < 0.6)
    w[:, 0] += 0.25
    soft[:, allowed] = w / w.sum(1, keepdim=True)
    return glabels, soft


def case(name, x, go, G, glabels, gsoft, keep=None, gscale=1.0, row_g=None):
    return dict(name=name, x=x, group_of=go, G=G, glabels=glabels, gsoft=gsoft, keep=keep, gscale=gscale, row_g=row_g)


def spread(name, C, G, seed):
    """logits uniform in [-1, 1], +120 on the classes of one group and -120 on those of the TARGET group: the row maximum lies 240
    above every member of the target, exp(x - row max) is 0 there in fp32 -- lse_g must come from the group's own maximum"""
    g = gen(seed)
    go = random_map(C, G, g, ungrouped=0.1 if C > G else 0.0)
    rows = 4
    x = torch.rand(rows, C, generator=g) * 2 - 1
    glabels = torch.arange(rows) % G
    high = (glabels + 1 + torch.arange(rows) % max(G - 1, 1)) % G
    soft = torch.zeros(rows, G)
    for r in range(rows):
        x[r, go == high[r]] += 120.0
        x[r, go == glabels[r]] -= 120.0
        soft[r, glabels[r]] = 0.75
        soft[r, high[r]] += 0.25
    return case(name, x, go, G, glabels, soft)


def build_cases():
    out = []
    g = gen(1)
    out.append(case("C1_G1", torch.randn(3, 1, generator=g) * 3, torch.zeros(1, dtype=torch.int64), 1, torch.tensor([0, -1, 0]),
                    torch.tensor([[1.0], [0.5], [2.0]])))
    # the second trip of the 256-stride column loop and of the 4-wave group loop; ungrouped classes; -1 labels
    g = gen(2)
    go = random_map(257, 5, g, ungrouped=0.2)
    gl, gs = targets(7, 5, g)
    gl[3] = -1
    out.append(case("C257_G5", torch.randn(7, 257, generator=g) * 3, go, 5, gl, gs, gscale=0.37, row_g=torch.randn(7, generator=g) + 0.2))
    # groups of 1, 65 and 300 members, an empty group that no row targets, and rows whose arg-max is an ungrouped class
    go, G = sized_map()
    g = gen(3)
    x = torch.randn(6, 400, generator=g) * 3
    x[1::2, torch.nonzero(go == -1)[0, 0]] += 20.0
    gl, gs = targets(6, G, g, allowed=[0, 1, 2])
    out.append(case("sizes_1_65_300", x, go, G, gl, gs))
    keep = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8)
    out.append(case("sizes_keep", x, go, G, gl, gs, keep=keep, gscale=2.5, row_g=torch.randn(6, generator=g) - 0.4))
    # G = 1 with every class grouped: the loss is 0 and so is the gradient (an identity, checked as such in the GPU tests)
    g = gen(4)
    out.append(case("G1_all", torch.randn(3, 130, generator=g) * 3, torch.zeros(130, dtype=torch.int64), 1, torch.zeros(3, dtype=torch.int64),
                    torch.tensor([[1.0], [0.3], [1.0]])))
    # G = C: every class its own group -- the plain cross-entropy
    g = gen(5)
    gl, gs = targets(5, 257, g)
    out.append(case("G_is_C", torch.randn(5, 257, generator=g) * 3, torch.randperm(257, generator=g), 257, gl, gs,
                    row_g=torch.randn(5, generator=g)))
    # the most groups the kernel takes
    g = gen(6)
    gl, gs = targets(2, 1024, g)
    out.append(case("G1024", torch.randn(2, 1500, generator=g) * 3, random_map(1500, 1024, g, ungrouped=0.1), 1024, gl, gs))
    # the workload's width: the action classes and the nouns of EPIC-KITCHENS-100
    g = gen(7)
    gl, gs = targets(3, 300, g)
    out.append(case("C3806_G300", torch.randn(3, 3806, generator=g) * 3, random_map(3806, 300, g), 300, gl, gs, gscale=0.5))
    out.append(spread("spread_C257_G5", 257, 5, 8))
    out.append(spread("spread_C400_G3", 400, 3, 9))
    return out


def build_bad_cases():
    """rows that must come out NaN (listed in `bad_hard` / `bad_soft`) among rows that must not notice"""
    go, G = sized_map()
    g = gen(20)
    x = torch.randn(6, 400, generator=g) * 3
    gl, gs = targets(6, G, g, allowed=[0, 1, 2])
    gl[1], gl[2], gl[4] = 3, G, -2              # the empty group, one past the last group, below -1
    gl[5] = -1                                  # ... and an ignored row, which stays exactly 0
    gs[0, 3] = 0.125                            # mass on the empty group
    gs[3, 3] = -1e-30                           # any non-zero mass
    c = case("bad_rows", x, go, G, gl, gs)
    c.update(bad_hard=[1, 2, 4], bad_soft=[0, 3])
    return [c]


CASES = build_cases()
BAD_CASES = build_bad_cases()


def variants(c):
    """(kind, glabels, gsoft) of a case"""
    return (("hard", c["glabels"], None), ("soft", None, c["gsoft"]))


def launch(ops, c, kind, ld, bf16, fn=None):
    """one launch (loss and gradient together) of ops.softmax_ce_groups on a case: logits as the first C columns of a NaN-filled
    [rows, ld] buffer, the gradient into rows 1..rows of a sentinel-filled [rows + 2, ld] buffer, soft targets as the first G columns
    of a NaN-filled [rows, G + 3] buffer.  Returns loss [rows], the [rows, ld] gradient block (fp32, on the CPU) and whether the
    sentinel rows around it survived."""
    x, G = c["x"], c["G"]
    rows, C = x.shape
    xd = torch.full((rows, ld), float("nan"), dtype=F32, device=dev())
    xd[:, :C] = x.to(dev())
    groups = ops.group_csr(c["group_of"], G, device=dev())
    gsoft = None
    if kind == "soft":
        gsoft = torch.full((rows, G + 3), float("nan"), dtype=F32, device=dev())
        gsoft[:, :G] = c["gsoft"].to(dev())
        gsoft = gsoft[:, :G]
    rl = torch.full((rows,), SENT, device=dev())
    dbuf = torch.full((rows + 2, ld), SENT, dtype=torch.bfloat16 if bf16 else F32, device=dev())
    (fn or ops.softmax_ce_groups)(xd[:, :C], C, groups, glabels=to_dev(c["glabels"]) if kind == "hard" else None, gsoft=gsoft,
                                  keep=to_dev(c["keep"]), gscale=c["gscale"], row_g=to_dev(c["row_g"]), dlogits=dbuf[1:rows + 1],
                                  row_loss=rl)
    border = bool((dbuf[0] == SENT).all()) and bool((dbuf[-1] == SENT).all())
    return rl.cpu(), dbuf[1:rows + 1].float().cpu(), border
