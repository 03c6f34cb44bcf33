"""Running a plan's launch lists: in order on the caller's stream, or with the branch chains and the deferred weight-gradient groups on side
streams behind the events of their fork / join / wfork markers -- eagerly or under hipGraph capture, which records the same launches.
A mixin of ``engine.Plan`` (split out of engine.py in round 7).  Reference: model(x) and loss.backward(), src/utils/method.py:150-182."""
import torch

from . import _lib
from .graph import _Call, _Marker


class Runner:
    def _run_lanes(self, calls, stream):
        """Launch `calls` with the independent branch chains (stream lane > 0) on side streams: a lane's first launch
        after a fork waits for the fork's event on the main stream, the join makes the main stream wait for every lane
        used since; outside fork/join regions (and at the end of the slice) everything is ordered on the main stream.
        Works eagerly and under hipGraph capture (the side streams join the capture through the events)."""
        main = torch.cuda.current_stream()
        assert main.cuda_stream == stream, "lanes need the launch stream to be torch's current stream"
        ev, forked, used = None, set(), set()
        wev, wused = {}, set()                 # weight-gradient side streams: pending event per stream, streams used
        for c in calls:
            if isinstance(c, _Marker):
                if c.kind == "wfork":            # the deferred weight gradients that follow may start once their source
                    src = main if c.lane == 0 else self._lane_streams[c.lane]      # stream got here
                    wev[c.slane] = src.record_event()
                elif c.kind == "fork":
                    ev, forked = main.record_event(), set()
                elif not self._pack_marker(c.kind, main, self._pack_stream):       # a join
                    for L in used:
                        main.wait_stream(self._lane_streams[L])
                    ev, used = None, set()
                continue
            L = c.slane
            if L == 0:
                c(stream)
                continue
            if L < 0:                          # deferred weight-gradient group
                s = self._lane_streams[L]
                e = wev.pop(L, None)
                if e is not None:
                    s.wait_event(e)
                elif L not in wused:
                    s.wait_stream(main)        # slice starts inside a group (data-parallel segments)
                wused.add(L)
                c(s.cuda_stream)
                continue
            s = self._lane_streams.get(L)
            if s is None:
                s = self._lane_streams[L] = torch.cuda.Stream()
            if L not in forked:
                if ev is not None:
                    s.wait_event(ev)
                else:
                    s.wait_stream(main)
                forked.add(L)
            used.add(L)
            c(s.cuda_stream)
        for L in used | wused:
            main.wait_stream(self._lane_streams[L])

    def _mirrored_forward(self):
        """The forward list with the image launch replaced by lh_nhwc4_mirror on img_nhwc4: the pass reads the input of the
        previous forward mirrored horizontally (flip test, runtime.InferStep(flip_test=True)); the rest of the list is the
        plain pass's, so a training-mode plan normalises with this pass's batch statistics and updates the running ones again."""
        i = self._image_call_index
        img = self.fwd[i]
        assert isinstance(img, _Call) and img.args[1] == self.img_nhwc4.data_ptr(), "the image launch moved in the forward list"
        self._mirror_call.slane = img.slane
        return self.fwd[:i] + [self._mirror_call] + self.fwd[i + 1:]

    def run_forward(self, stream, mirrored=False):
        """mirrored=True: the forward of the horizontal mirror of the image the previous forward read (_mirrored_forward)."""
        calls = self._mirrored_forward() if mirrored else self.fwd
        if self.use_lanes:
            return self._run_lanes(calls, stream)
        for c in calls:
            if not isinstance(c, _Marker):
                c(stream)
            else:                                # no side streams in this plan: a late pack group runs in place
                self._pack_marker(c.kind, torch.cuda.current_stream(), None)

    def run_backward(self, stream, lo=0, hi=None):
        """Run bwd[lo:hi] (a segment of the backward list: data-parallel plans replay it bucket by bucket)."""
        calls = self.bwd[lo:hi]
        if self.use_lanes:
            return self._run_lanes(calls, stream)
        for c in calls:
            if not isinstance(c, _Marker):
                c(stream)

    def forward(self, images, repack=True):
        """images: fp32 NCHW on the device.  Returns the plan's fp32 NCHW heatmap buffer."""
        if tuple(images.shape) != (self.n, 3, self.h, self.w):
            raise _lib.LightHandError(f"plan was built for {(self.n, 3, self.h, self.w)}, got {tuple(images.shape)}")
        self.img_nchw.copy_(images)
        stream = torch.cuda.current_stream().cuda_stream
        if repack:
            self.refresh_packs(stream)
        self.run_forward(stream)
        return self.out_nchw

    def backward(self, dheat):
        self.dout_nchw.copy_(dheat)
        self.run_backward(torch.cuda.current_stream().cuda_stream)
