/*
   filter.pict.hip.swift — PictureFilter for the HIP backend (source only: no Swift toolchain in the
   build container; the same operator is exercised through swiftvideo_amd/compute.py::PictureFilter and
   swiftvideo_amd/host/swiftvideo_hip.hpp::PictureFilter, tests/test_gpu_mixer.py, tests/cpp/).

   The reference declares this operator and leaves it commented out
   (Sources/SwiftVideo/filter.pict.swift:20-47): a Tx<PictureSample, PictureSample> with a compute
   context of its own.  This file gives it a body: convert a picture to `outputFormat` at `outputSize`
   on the device — one full-canvas layer through the composite kernels (colour conversion + bilinear
   scale in one launch) or a separable Lanczos-3 resample: without conversion (BGRA -> BGRA, nv12 -> nv12,
   y420p -> y420p; chv_scale_lanczos, a 4:2:0 picture plane by plane), or BGRA / RGBA -> nv12 / y420p through
   the integer matrix (chv_scale_lanczos_to_yuv), or — only with convert420 — nv12 <-> y420p, the logical planes
   resampled one by one and stored in the other packing (chv_scale_lanczos_420), or — only with convertToRgb — nv12 / y420p ->
   BGRA / RGBA through the integer matrix (chv_scale_lanczos_from_yuv).
   It replaces filter.pict.swift when GPGPU_HIP is defined.
*/
#if GPGPU_HIP
import Foundation
import VectorMath
import CHIPVideo

public enum PictureScaler {
    case bilinear
    case lanczos
}

public class PictureFilter: Tx<PictureSample, PictureSample> {
    public init(_ clock: Clock,
                outputSize: Vector2,
                outputFormat: PixelFormat = .BGRA,
                scaler: PictureScaler = .bilinear,
                integerMatrix: Bool = true,
                colorspace: Int32 = 0,
                convert420: Bool = false,
                convertToRgb: Bool = false,
                convertDecoderFormats: Bool = false,
                convertHighBitDepth: Bool = false,
                computeContext: ComputeContext? = nil) {
        self.clock = clock
        self.outputSize = outputSize
        self.outputFormat = outputFormat
        self.scaler = scaler
        self.integerMatrix = integerMatrix
        self.colorspace = colorspace
        self.convert420 = convert420
        self.convertToRgb = convertToRgb
        self.convertDecoderFormats = convertDecoderFormats
        self.convertHighBitDepth = convertHighBitDepth
        do {
            if let context = computeContext {
                self.context = createComputeContext(sharing: context)
            } else {
                self.context = try makeComputeContext(forType: .GPU)
            }
        } catch {
            self.context = nil
        }
        super.init()
        super.set { [weak self] sample in
            guard let strongSelf = self else {
                return .gone
            }
            guard let ctx = strongSelf.context else {
                return .error(EventError("filter.pict", -1, "No Compute Context", assetId: sample.assetId()))
            }
            do {
                // CPU samples are uploaded first (what GPUBarrierUpload would do, compute.swift:175-198)
                let src = sample.bufferType() == .cpu ? try uploadComputePicture(ctx, pict: sample) : sample
                let dst = try strongSelf.getBacking(ctx, like: sample)
                strongSelf.context = try usingContext(ctx) {
                    switch strongSelf.scaler {
                    case .lanczos:
                        let format = strongSelf.outputFormat
                        let rgbIn = src.pixelFormat() == .BGRA || src.pixelFormat() == .RGBA
                        if strongSelf.integerMatrix && rgbIn && (format == .nv12 || format == .y420p) {
                            // (the float full-range matrix has no Lanczos form)
                            return try scaleLanczosToYuv($0, src: src, target: dst, colorspace: strongSelf.colorspace)
                        }
                        let yuvIn = src.pixelFormat() == .nv12 || src.pixelFormat() == .y420p
                        if strongSelf.convert420 && yuvIn && (format == .nv12 || format == .y420p) && src.pixelFormat() != format {
                            return try scaleLanczos420($0, src: src, target: dst)
                        }
                        let decoderIn = [PixelFormat.nv21, .y422p, .y444p, .yuvs, .zvuy].contains(src.pixelFormat())
                        if strongSelf.convertDecoderFormats && decoderIn && (format == .nv12 || format == .y420p) {
                            return try scaleLanczosTo420($0, src: src, target: dst)
                        }
                        let hbdIn = src.pixelFormat() == .p010 || src.pixelFormat() == .y420p10
                        if strongSelf.convertHighBitDepth && hbdIn && (format == .nv12 || format == .y420p) {
                            return try scaleLanczosHbdTo420($0, src: src, target: dst)
                        }
                        if strongSelf.convertToRgb && yuvIn && (format == .BGRA || format == .RGBA) {
                            return try scaleLanczosFromYuv($0, src: src, target: dst, colorspace: strongSelf.colorspace)
                        }
                        guard src.pixelFormat() == format, format == .BGRA || format == .nv12 || format == .y420p else {
                            throw ComputeError.notImplemented
                        }
                        return try scaleLanczos($0, src: src, target: dst)
                    case .bilinear:
                        // the unit quad stretched over the whole canvas (what PictureAnimator produces for a
                        // picture at the origin with the canvas' size), no border, no fill, opaque
                        let quad = Matrix4(outputSize) * Matrix4(scale: Vector3(outputSize.x, outputSize.y, 1))
                        let full = PictureSample(src, matrix: quad, textureMatrix: Matrix4.identity,
                                                 borderMatrix: quad, fillColor: Vector4(0, 0, 0, 0), opacity: 1.0)
                        let cleared = try runComputeKernel($0, images: [PictureSample](), target: dst,
                                                           kernel: strongSelf.findKernel(nil))
                        return try applyComputeImage(cleared, image: full, target: dst,
                                                     kernel: strongSelf.findKernel(src))
                    }
                }
                // time stamps, ids and transform state of the incoming sample carry over; only the image changes
                return .just(PictureSample(sample, img: dst.imageBuffer()))
            } catch let error {
                return .error(EventError("filter.pict", -2, "Compute error \(error)", assetId: sample.assetId()))
            }
        }
    }

    // same naming rule as VideoMixer.findKernel (mix.video.swift:142-146); BGRA targets take the
    // transform-aware kernels of the HIP backend
    private func findKernel(_ image: PictureSample?) throws -> ComputeKernel {
        let inp = image <??> { String(describing: $0.pixelFormat()).lowercased() } <|> "clear"
        let outp = String(describing: outputFormat).lowercased()
        let rgbIn = image != nil && (inp == "bgra" || inp == "rgba")
        // BGRA targets: the transform-aware kernels; 4:2:0 targets from RGB pictures: the integer BT.601/709 matrix
        // (img_*_int, what an encoder expects; the default, as in swiftvideo_amd/compute.py::PictureFilter and
        // host/swiftvideo_hip.hpp) — or, with integerMatrix: false, the reference's own float full-range rows
        // (kernels.cl.swift:96-99), byte for byte what its OpenCL family writes
        let to420 = outp == "nv12" || outp == "y420p"
        let suffix = (rgbIn && outp == "bgra") ? "_tx" : (rgbIn && to420 && integerMatrix) ? "_int" : ""
        return try defaultComputeKernelFromString("img_\(inp)_\(outp)\(suffix)")
    }

    // ring of device images, as VideoMixer.getBacking (mix.video.swift:148-167)
    private func getBacking(_ ctx: ComputeContext, like: PictureSample) throws -> PictureSample {
        if backing.count < numberBackingImages {
            let image = try createPictureSample(outputSize, outputFormat,
                                                assetId: like.assetId(), workspaceId: like.workspaceId())
            let gpuImage = try uploadComputePicture(ctx, pict: image)
            backing.append(gpuImage)
            return gpuImage
        }
        let image = backing[currentBacking]
        currentBacking = (currentBacking + 1) % backing.count
        return image
    }

    private let numberBackingImages = 10
    private var backing = [PictureSample]()
    private var currentBacking = 0
    let clock: Clock
    let outputSize: Vector2
    let outputFormat: PixelFormat
    let scaler: PictureScaler
    let integerMatrix: Bool
    let colorspace: Int32      // chv_colorspace of the integer matrix (the Lanczos conversion)
    let convert420: Bool       // the Lanczos scaler takes nv12 <-> y420p (off: the pair is an error, as it was)
    let convertToRgb: Bool     // the Lanczos scaler takes nv12 / y420p -> BGRA / RGBA (off: the pair is an error, as it was)
    let convertDecoderFormats: Bool      // the Lanczos scaler takes nv21 / y422p / y444p / yuvs / zvuy -> nv12 / y420p (off: an error, as it was)
    let convertHighBitDepth: Bool        // the Lanczos scaler takes p010 / y420p10 -> nv12 / y420p (off: an error, as it was)
    var context: ComputeContext?
}
#endif
