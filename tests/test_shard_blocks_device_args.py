"""mrt.dist.shard_blocks_device validates its arguments like the host shard_blocks: a
non-positive block and an owners array that is not one entry per block raise ValueError;
valid calls deal what shard_blocks deals."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from mrt.dist import balance_blocks, shard_blocks, shard_blocks_device  # noqa: E402


@pytest.mark.parametrize("block", [0, -5])
def test_non_positive_block_is_a_value_error(block):
    with pytest.raises(ValueError, match="block must be positive"):
        shard_blocks_device(1000, 2, 0, block, device="cpu")
    with pytest.raises(ValueError):
        shard_blocks(1000, 2, 0, block)                       # the host deal's behaviour it matches


@pytest.mark.parametrize("delta", [-1, 1])
def test_owners_of_the_wrong_length_is_a_value_error(delta):
    n, block = 1000, 64                                       # 16 blocks
    owners = np.arange(16 + delta) % 2
    with pytest.raises(ValueError, match="block owners"):
        shard_blocks_device(n, 2, 0, block, owners=owners, device="cpu")
    with pytest.raises(ValueError):
        shard_blocks(n, 2, 0, block, owners=owners)


@pytest.mark.parametrize("n,block,world", [(1000, 64, 2), (4096, 64, 3), (77, 100, 2), (8, 8, 2)])
def test_valid_calls_are_unchanged(n, block, world):
    """Cyclic and owner deals, in frame order and by priority, equal the host shard_blocks;
    the ray count is the blocks' rays (the frame's partial last block counted short)."""
    nblocks = -(-n // block)
    rng = np.random.default_rng(7)
    prio = rng.integers(0, 5, size=nblocks)
    owners = balance_blocks(prio, world)
    for rank in range(world):
        for own in (None, owners):
            for pr in (None, prio):
                got, rays = shard_blocks_device(n, world, rank, block, owners=own,
                                                priority=None if pr is None else torch.from_numpy(pr), device="cpu")
                want = shard_blocks(n, world, rank, block, owners=own, priority=pr)
                assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
                assert rays == int(sum(min(n, (b + 1) * block) - b * block for b in want))
