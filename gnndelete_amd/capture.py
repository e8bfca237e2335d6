"""hipGraph capture of a training iteration that must not move the trajectory (NodeembEngine, EdgeprobEngine)."""
import torch


def capture_iterations(iteration, mutable_state, k=1, warm_up=True):
    """-> torch.cuda.CUDAGraph of k calls of iteration(), ready to replay; the tensors mutable_state() lists are left as found.
    warm_up: one eager iteration on a side stream first (allocator, code objects, the plans' cached work items).  The first
    launch of a graph exec uploads it to the device (tens of us): it is done here, on state that is restored right after, so a
    short run does not pay it."""
    saved = [t.clone() for t in mutable_state()]
    if warm_up:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            iteration()
        torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(k):
            iteration()
    graph.replay()
    torch.cuda.synchronize()
    for t, s in zip(mutable_state(), saved):
        t.copy_(s)                             # undo the warm-up and the upload replay
    return graph
