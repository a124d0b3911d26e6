/*
   mixgroup.hip.swift — many mixer ticks in ONE launch for the HIP backend (source only: no Swift toolchain in the build
   container; the same two classes are exercised through swiftvideo_amd/compute.py::TickBatch / VideoMixerGroup and
   swiftvideo_amd/host/swiftvideo_hip.hpp, tests/test_gpu_mixer.py, tests/cpp/).

   Why it exists.  VideoMixer.mix (mix.video.swift:95-140) issues, per mixer and per tick, a clear, one kernel per layer
   and one blocking wait (usingContext, compute.swift:131-134).  On an MI355X one 720p tick is ~7 us of device work behind
   a ~14 us launch + wait floor (tools/tick_latency.py): a composer with many mixers on one device
   (composer.swift:203-224) leaves the device idle most of the time.  With the two hunks of INTEGRATION.md section 1
   a mixer (a) issues its tick as one chv_composite launch, or (b) — when it belongs to a VideoMixerGroup — hands the
   tick to the group, which composes the ticks of all its members with ONE chv_batch launch per canvas format and ONE
   host wait.  Current figures: INTEGRATION.md section 1 and the `workloads` of the default bench.py line (round 3: 256
   ticks per launch = 4.9 us of device time per tick; one tick at a time 23-25 us fused, 54-56 us as the unchanged
   clear + 4 launches sequence: legs pipeline_per_tick / pipeline_reference_sequence).  The per-tick figure of a group does
   not include building the TickBatch: VideoMixerGroup.flush below makes a new one every tick unless the group was made with
   `reuseBatches: true` — then it keeps one batch per canvas format with the signature of its scene and points it at every tick's
   pictures (TickBatch.rebind -> chv_batch_rebind: the upload ring and the ring of 10 canvases, mix.video.swift:148-165, rotate
   every tick, and nothing but plane addresses changes between two ticks of a scene); figures in profiles/batch_rebind_notes.md.
*/
#if GPGPU_HIP
import Foundation
import Dispatch
import VectorMath
import CHIPVideo

/// One mixer tick: clear the target, then the layers in z order (mix.video.swift:116-124).
public struct MixTick {
    public let target: PictureSample
    public let clearFirst: Bool
    public let layers: [(PictureSample, ComputeKernel, ImageUniforms)]
    public init(target: PictureSample, clearFirst: Bool = true, layers: [(PictureSample, ComputeKernel, ImageUniforms)]) {
        self.target = target
        self.clearFirst = clearFirst
        self.layers = layers
    }
}

/// N independent ticks of one canvas format as ONE kernel launch (chv_batch_create / chv_batch_run).  The descriptors
/// live on the device until `deinit`; the pictures a batch refers to are retained by it.  Byte-identical to running the
/// ticks one by one through compositeTick or through clear + applyComputeImage.
public final class TickBatch {
    public let count: Int
    public private(set) var kernelName = ""
    private var handle: OpaquePointer?
    private var retained: [PictureSample]

    public init(_ context: ComputeContext, ticks: [MixTick]) throws {
        guard !ticks.isEmpty else {
            throw ComputeError.invalidValue
        }
        // chv_tick holds a pointer to its layers: keep every tick's layer array alive, at a stable address, until
        // chv_batch_create has copied the descriptors to the device
        var layerStorage = [UnsafeMutablePointer<chv_layer>]()
        defer { layerStorage.forEach { $0.deallocate() } }
        var descs = [chv_tick]()
        var keep = [PictureSample]()
        for tick in ticks {
            guard let targetImage = tick.target.imageBuffer(), let targetDesc = describeImage(targetImage, maxPlanes: 3) else {
                throw ComputeError.badTarget
            }
            let storage = UnsafeMutablePointer<chv_layer>.allocate(capacity: max(tick.layers.count, 1))
            layerStorage.append(storage)
            for (index, (sample, kernel, uniforms)) in tick.layers.enumerated() {
                storage[index] = try makeLayer(sample, kernel, uniforms)
                keep.append(sample)
            }
            var desc = chv_tick()
            desc.target = targetDesc
            desc.clear_first = tick.clearFirst ? 1 : 0
            desc.n_layers = Int32(tick.layers.count)
            desc.layers = UnsafePointer(storage)
            descs.append(desc)
            keep.append(tick.target)
        }
        var batch: OpaquePointer?
        try checkStatus(chv_batch_create(context.handle, &descs, Int32(descs.count), &batch))
        self.handle = batch
        self.count = ticks.count
        self.retained = keep
        var name = [CChar](repeating: 0, count: 128)
        if chv_batch_describe(batch, &name, 128, nil) == 0 {
            self.kernelName = String(cString: name)
        }
    }

    /// Enqueue the whole batch on the context's stream (inside a compute pass, like runComputeKernel).
    public func run(_ context: ComputeContext) throws -> ComputeContext {
        try checkStatus(chv_batch_run(context.handle, handle))
        return context
    }

    /// Point the batch at the pictures of `ticks` (chv_batch_rebind): the same scene — kernels, uniforms, plane sizes and pitches —
    /// over other memory.  Anything else throws and leaves the batch as it was.  Ordered on the context's stream like `run`.
    public func rebind(_ context: ComputeContext, ticks: [MixTick]) throws -> ComputeContext {
        var items = [chv_rebind]()
        var keep = [PictureSample]()
        for (index, tick) in ticks.enumerated() {
            guard let targetImage = tick.target.imageBuffer(), let targetDesc = describeImage(targetImage, maxPlanes: 3) else {
                throw ComputeError.badTarget
            }
            items.append(chv_rebind(tick: Int32(index), layer: -1, image: targetDesc))
            keep.append(tick.target)
            for (position, (sample, _, _)) in tick.layers.enumerated() {
                guard let image = sample.imageBuffer(), let desc = describeImage(image, maxPlanes: 3) else {
                    throw ComputeError.badInputData(description: "Bad input image")
                }
                items.append(chv_rebind(tick: Int32(index), layer: Int32(position), image: desc))
                keep.append(sample)
            }
        }
        try checkStatus(chv_batch_rebind(context.handle, handle, &items, Int32(items.count)))
        retained = keep                       // (the pictures rebound away are released: the runs that read them were issued before)
        return context
    }

    /// What a batch is built from with the pictures' addresses left out: per tick the kernel ids, the 236 uniform bytes, clear_first,
    /// and per picture its format, plane sizes, pitches and components.  Equal signatures: `rebind`; anything else: a new batch.
    public static func sceneSignature(_ ticks: [MixTick]) throws -> Data {
        var signature = Data()
        func append<T>(_ value: T) {
            var v = value
            withUnsafeBytes(of: &v) { signature.append(contentsOf: $0) }
        }
        func picture(_ sample: PictureSample) throws {
            guard let image = sample.imageBuffer(), let desc = describeImage(image, maxPlanes: 3) else {
                throw ComputeError.badInputData(description: "Bad input image")
            }
            append(desc.format); append(desc.width); append(desc.height); append(desc.n_planes)
            for plane in [desc.planes.0, desc.planes.1, desc.planes.2] {
                append(plane.width); append(plane.height); append(plane.pitch); append(plane.components)
            }
        }
        for tick in ticks {
            try picture(tick.target)
            append(tick.clearFirst); append(Int32(tick.layers.count))
            for (sample, kernel, uniforms) in tick.layers {
                let layer = try makeLayer(sample, kernel, uniforms)
                append(layer.kernel); append(layer.uniforms); append(layer.opts.colorspace)
                try picture(sample)
            }
        }
        return signature
    }

    deinit {
        if let batch = handle {
            _ = chv_batch_destroy(batch)      // safe from any thread; selects the device itself
        }
    }
}

/// Several VideoMixers of one device ticked together.  Members keep their own samples, backing ring and z order
/// (mix.video.swift:57-75,148-165); what changes is WHO launches: a member that belongs to a group calls
/// `submit(...)` from its `mix(at:)` (the mix.video.swift hunk in INTEGRATION.md section 1) instead of launching, and the
/// group composes all ticks submitted for one clock time with one launch per canvas format and one host wait, then
/// runs every member's completion (which emits the member's PictureSample exactly as the unchanged code does).
public final class VideoMixerGroup {
    /// `reuseBatches`: keep one batch per canvas format with its scene signature; a tick of the same signature rebinds every picture and
    /// runs, any difference — or a refused rebind — builds afresh.  Same bytes either way; off by default.
    public init(_ context: ComputeContext, members: Int, flushAfter: DispatchTimeInterval = .milliseconds(2), reuseBatches: Bool = false) {
        self.context = createComputeContext(sharing: context)
        self.members = members
        self.flushAfter = flushAfter
        self.reuseBatches = reuseBatches
        self.queue = DispatchQueue(label: "mix.video.group")
    }

    /// Called by a member mixer on its own queue.  `completion` receives nil on success or the error that made the
    /// group's launch fail (the member turns it into EventError("mix.video", -2, …) as mix.video.swift:133-137 does).
    public func submit(time: TimePoint, tick: MixTick, completion: @escaping (Error?) -> Void) {
        queue.async { [weak self] in
            guard let strongSelf = self else {
                return
            }
            strongSelf.pending[time.value, default: []].append((tick, completion))
            if strongSelf.pending[time.value]?.count == strongSelf.members {
                strongSelf.flush(time.value)
            } else if strongSelf.pending[time.value]?.count == 1 {
                // a member that misses a tick (no context, torn down) must not hold the others back
                strongSelf.queue.asyncAfter(deadline: .now() + strongSelf.flushAfter) { [weak self] in
                    self?.flush(time.value)
                }
            }
        }
    }

    private func flush(_ time: Int64) {
        guard let ticks = pending.removeValue(forKey: time), let ctx = context else {
            return
        }
        var failure: Error?
        do {
            // a batch is one kernel family: one batch per canvas format, all enqueued in one pass, one wait
            var byFormat = [String: [MixTick]]()
            for (tick, _) in ticks {
                byFormat[String(describing: tick.target.pixelFormat()), default: []].append(tick)
            }
            let batches = try byFormat.map { try reuseBatches ? batch(ctx, format: $0.key, ticks: $0.value) : TickBatch(ctx, ticks: $0.value) }
            context = try usingContext(ctx) { try batches.reduce($0) { try $1.run($0) } }
        } catch let error {
            failure = error
        }
        ticks.forEach { $0.1(failure) }
    }

    /// the kept batch of this canvas format pointed at `ticks`, or a new one (kept in its place)
    private func batch(_ ctx: ComputeContext, format: String, ticks: [MixTick]) throws -> TickBatch {
        let signature = try TickBatch.sceneSignature(ticks)
        if let (keptSignature, keptBatch) = kept[format], keptSignature == signature {
            do {
                _ = try keptBatch.rebind(ctx, ticks: ticks)
                return keptBatch
            } catch {
                // (say, a picture at an address of another alignment: a new batch takes whatever it is given)
            }
        }
        let fresh = try TickBatch(ctx, ticks: ticks)
        kept[format] = (signature, fresh)
        return fresh
    }

    deinit {
        kept.removeAll()
        if let ctx = context {
            try? destroyComputeContext(ctx)
        }
    }

    private var context: ComputeContext?
    private let reuseBatches: Bool
    private var kept = [String: (Data, TickBatch)]()
    private let members: Int
    private let flushAfter: DispatchTimeInterval
    private let queue: DispatchQueue
    private var pending = [Int64: [(MixTick, (Error?) -> Void)]]()
}

// MARK: - shared with compute.hip.swift (which keeps its own private copies of describe / check for the contract functions)

/// `ImageUniforms` of a layer exactly as applyComputeImage builds them (compute.swift:149-161).
public func imageUniforms(for image: PictureSample, target: PictureSample) -> ImageUniforms {
    ImageUniforms(transform: image.matrix().inverse.transpose,
                  textureTransform: image.textureMatrix().inverse.transpose,
                  borderMatrix: image.borderMatrix().inverse.transpose,
                  fillColor: image.fillColor(),
                  inputSize: Vector2([image.size().x, image.size().y]),
                  outputSize: Vector2([target.size().x, target.size().y]),
                  opacity: image.opacity(),
                  imageTime: seconds(image.time()),
                  targetTime: seconds(target.time()))
}

private func checkStatus(_ status: Int32) throws {
    if status != 0 {
        throw computeError(fromStatus: status)          // compute.hip.swift: chv_status -> ComputeError, case by case
    }
}

private func makeLayer(_ sample: PictureSample, _ kernel: ComputeKernel, _ uniforms: ImageUniforms) throws -> chv_layer {
    guard let image = sample.imageBuffer(), let desc = describeImage(image, maxPlanes: 3) else {
        throw ComputeError.badInputData(description: "Bad input image")
    }
    var layer = chv_layer()
    layer.kernel = try kernelIdentifier(kernel)         // compute.hip.swift: ComputeKernel -> chv_kernel by name
    layer.image = desc
    var u = uniforms
    withUnsafeBytes(of: &u) { src in
        withUnsafeMutableBytes(of: &layer.uniforms) { $0.copyMemory(from: UnsafeRawBufferPointer(rebasing: src[0..<236])) }
    }
    return layer
}
#endif
